"""The fused chain kernel of MCMC.gp_mh(chains=, fused=True) on the device (cesx_gp_run, gp_chain_kernel: K Metropolis steps
on the emulator per launch): the real reference's chains, the step path under the same device noise at the tile's and the
panel's edges, phi, alternation with single steps, injected noise, the fp32 engine, a shard, variances <= 0 and the error
returns.  The cases and their numpy restatement: tests/gp_chain_cases.py (their decisions are checked to sit away from
rounding in tests/test_gp_chain_host.py)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_emulate_host import gold_call, gold_prior, gold_problem, load_gold  # noqa: E402
from gp_cases import random_gps  # noqa: E402
import gp_chain_cases as gc  # noqa: E402

pytestmark = pytest.mark.gpu
K_STEPS = gc.K_STEPS
CASES = gc.cases()


def _bound(samples, K=K_STEPS):
    return 4 * K * 2.0 ** -52 * max(1.0, float(np.max(np.abs(samples))))


# ---- 1. the reference's chains ---------------------------------------------------------------------------------------

DEVICE_CASES = [c["name"] for c in load_gold()[0]["cases"] if c["name"] not in ("pca", "compounded_dense")]


@pytest.mark.parametrize("case", DEVICE_CASES)
def test_fused_chains1_reproduces_reference(case):
    """Every golden case the step path runs on the device (tests/test_gpu_gp.py), through the fused kernel with the
    reference's numpy draws: the reference's samples at rtol = atol = 1e-10, its accept rate at 1e-12."""
    from ces_amd import sample
    man, a = load_gold()
    c = [c for c in man["cases"] if c["name"] == case][0]
    enka = gold_problem(a, c["scaled"])
    mc = sample.MCMC()
    mc.mute_bar, mc.y_obs, mc.noise = True, a["prob_y"], "numpy"
    np.random.seed(c["seed"])
    call = gold_call(a, c["kwargs"])
    legs = [c["resume"], man["STEPS"] - c["resume"]] if c["resume"] else [man["STEPS"]]
    for steps in legs:
        mc.gp_mh(enka, steps, gold_prior(a), chains=1, fused=True, **call)
        assert mc.fused_launches >= 1
    np.testing.assert_allclose(mc.samples, a["mh_%s_samples" % case], rtol=1e-10, atol=1e-10)
    assert abs(mc.accept - float(a["mh_%s_accept" % case])) < 1e-12


# ---- 2. fused equals the step path ---------------------------------------------------------------------------------------

def _sampler(c, noise="device"):
    from ces_amd import sample
    enka, y, prior, kw = gc.problem(c)
    mc = sample.MCMC()
    mc.mute_bar, mc.y_obs, mc.noise, mc.seed = True, y, noise, gc.SEED
    return mc, enka, prior, kw


def _run(c, fused, n_mcmc, stride, start_step=0, noise="device", seed=None):
    """One run: (sampler, the samples of the last call (p, kept, M), the per-chain accept counters)."""
    mc, enka, prior, kw = _sampler(c, noise)
    mc.trace_stride = stride
    if seed is not None:
        np.random.seed(seed)
    if start_step:                                         # the resume path: the first leg on the step path for both
        mc.gp_mh(enka, start_step, prior, chains=c["M"], fused=False, **kw)
        assert mc._mh_next_step == start_step and mc.fused_launches == 0
    first = 0 if not start_step else mc.samples.shape[1]
    mc.gp_mh(enka, n_mcmc, prior, chains=c["M"], fused=fused, **kw)
    assert mc.fused_launches == (1 if fused else 0)
    samples = mc.samples.reshape(c["p"], mc.samples.shape[1], c["M"])
    return mc, samples[:, first:, :], np.rint(np.asarray(mc.accept_chains) * n_mcmc).astype(np.int64)


@pytest.mark.parametrize("c", CASES, ids=gc.case_id)
def test_fused_equals_the_step_path(c):
    """Same seed, device noise, K = 7 steps, stride 1 and 3, from step 0 and from step 5 through the resume path: the
    per-chain accept counters are equal (no chain excluded: tests/test_gp_chain_host.py keeps every decision of these cases
    1e-7 away from its threshold), the kept samples have the same shape and agree within 4 K 2^-52 max(1, max|U|) (two ulp
    per proposal for the differing order of its products, accumulated over K steps), ``samples_device`` is the last kept
    state bit for bit and mh_stats reports K steps.  mh_phi() after the fused run is the fp64 numpy phi of the final states
    within 1e-9 of the sum of its absolute terms (the bar tests/test_gpu_gp.py holds the prediction to)."""
    p, M = c["p"], c["M"]
    for stride in (1, 3):
        for start_step in (0, 5):
            _, a, ca = _run(c, False, K_STEPS, stride, start_step)
            mc, b, cb = _run(c, True, K_STEPS, stride, start_step)
            case = (stride, start_step)
            assert a.shape == b.shape == (p, (0 if start_step else 1) + K_STEPS // stride + (1 if K_STEPS % stride else 0), M), case
            err = float(np.max(np.abs(a - b)))
            print("\n[gp chain] fused vs step %s stride=%d start=%d: max err %.3g (bound %.3g), accepted %d of %d"
                  % (gc.case_id(c), stride, start_step, err, _bound(a), ca.sum(), K_STEPS * M))
            assert np.array_equal(ca, cb), case
            if M >= 31:
                assert 0 < ca.sum() < K_STEPS * M             # proposals are accepted and rejected alike
            assert err <= _bound(a), case
            final = np.ascontiguousarray(b[:, -1, :])
            assert np.array_equal(mc.samples_device.cpu().numpy(), final)
            steps, _, per = mc._mh_eng.mh_stats(per_chain=True)
            assert steps == K_STEPS and np.array_equal(per.astype(np.int64), cb)
            # 3. phi
            enka, y, prior, kw = gc.problem(c)
            phi, mag = gc.np_phi(enka, y, prior, kw, final)
            got = mc._mh_eng.mh_phi()
            assert np.all(np.abs(got - phi) <= 1e-9 * mag), (case, float(np.max(np.abs(got - phi) / mag)))


def test_fused_matches_the_numpy_chains():
    """The fused run against the fp64 numpy restatement under the same device noise (oracle/philox.py), one case per
    likelihood mode: equal accept counters, final states within 1e-9 (1 + |U|)."""
    for c in (CASES[3], CASES[4], CASES[10], CASES[18]):
        mc, b, cb = _run(c, True, K_STEPS, K_STEPS)
        Ur, acc, _, _ = gc.np_chains(c, K_STEPS)
        assert np.array_equal(cb, acc), gc.case_id(c)
        assert np.all(np.abs(b[:, -1, :] - Ur) <= 1e-9 * (1 + np.abs(Ur))), gc.case_id(c)


# ---- engines driven by hand --------------------------------------------------------------------------------------------

def _prepared_engine(c, J, dtype="float64", J_global=None, j_offset=0, cols=None, f32_start=False):
    """An engine with the problem, the proposal, the emulator and the start states of case ``c`` scored:
    (eng, U, mode, want_var, nugget)."""
    import torch
    from ces_amd import emulate, engine
    enka, y, prior, kw = gc.problem(c)
    p, n = enka.p, enka.n_obs
    eng = engine.Engine(p, n, J, dtype=dtype, J_global=J_global, j_offset=j_offset, seed=gc.SEED)
    Gamma = kw.get("Gamma", None)
    mode = "var" if Gamma is None else "gamma_var" if kw.get("noise_compounded") else "gamma"
    eng.set_problem(y, np.eye(n) if Gamma is None else Gamma, prior.mean, np.asarray(prior.cov).reshape(p, p), prior.mean)
    eng.mh_set_proposal(kw.get("update"), gc.scales_of(enka, kw), kw.get("beta", 0.5))
    eng.gp_set(emulate.device_image(enka, enka.gpmodels))
    rng = np.random.default_rng(9)
    U0 = enka.Ustar.mean(axis=1)[:, None] + 0.2 * rng.standard_normal((p, J_global or J))
    if f32_start:
        U0 = U0.astype(np.float32).astype(np.float64)
    if cols is not None:
        U0 = np.ascontiguousarray(U0[:, cols])
    U = eng.to_device(U0, p, "U0").clone()
    want_var = mode != "gamma"
    mean, var = eng.gp_predict(U, nugget=c["nugget"], var=want_var)
    eng.gp_start(mode, U, mean, var)
    torch.cuda.synchronize()
    return eng, U, mode, want_var, c["nugget"]


def test_fused_launches_and_single_steps_alternate():
    """A 4-step fused launch, one single step through mh_propose / gp_predict / gp_accept, 2 more fused steps: equal to 7
    single steps under the bound of the fused comparison, with equal counters; mh_stats reports 7 steps."""
    import torch
    c = dict(CASES[9], M=65)                               # gamma_var, the nugget, a dense prior, four GPs
    ends = []
    for mixed in (False, True):
        eng, U, mode, want_var, nugget = _prepared_engine(c, 65)
        P = eng.empty(c["p"])

        def single(step):
            eng.mh_propose(step, U, out=P)
            mean, var = eng.gp_predict(P, nugget=nugget, var=want_var)
            eng.gp_accept(mode, step, U, P, mean, var)
        if mixed:
            eng.gp_run(mode, 0, 4, U, nugget=nugget)
            single(4)
            eng.gp_run(mode, 5, 2, U, nugget=nugget)
        else:
            for step in range(7):
                single(step)
        steps, _, per = eng.mh_stats(per_chain=True)
        assert steps == 7
        torch.cuda.synchronize()
        ends.append((U.cpu().numpy(), per.copy(), eng.mh_phi()))
        eng.close()
    (Ua, ca, pa), (Ub, cb, pb) = ends
    assert np.array_equal(ca, cb) and 0 < ca.sum() < 7 * 65
    assert np.max(np.abs(Ua - Ub)) <= _bound(Ua)
    assert np.allclose(pa, pb, rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize("M", [1, 33])
def test_fused_with_injected_noise(M):
    """``noise='numpy'`` under one np.random.seed: fused=True equals fused=False under the bound of the fused comparison (the
    draws are stacked per launch in the step loop's order)."""
    for base in (CASES[4], CASES[8]):                       # gamma with a dense Gamma (p = 2); var, pCN (p = 5)
        c = dict(base, M=M)
        _, a, ca = _run(c, False, K_STEPS, 1, noise="numpy", seed=11)
        mc, b, cb = _run(c, True, K_STEPS, 1, noise="numpy", seed=11)
        assert mc.samples.shape == ((c["p"], K_STEPS + 1) if M == 1 else (c["p"], K_STEPS + 1, M))
        assert np.array_equal(ca, cb) and np.max(np.abs(a - b)) <= _bound(a)


def test_fp32_engine_is_the_fp64_launch_rounded_on_the_store():
    """One fused launch (K = 7, device noise, the same seed) on an fp32 and on an fp64 engine from start states exactly
    representable in fp32: within a launch all arithmetic is fp64 and both engines draw the same normals, so the fp32 trace
    and final U are the fp64 ones cast to float32 bit for bit and the counters are equal; a second identical launch on a
    fresh engine is bit-identical."""
    import torch
    J = 65
    for base in (CASES[2], CASES[9]):                       # var without the nugget (p = 5); gamma_var (p = 1, four GPs)
        c = dict(base, M=J)
        out = {}
        for key, dtype in (("f32", "float32"), ("f64", "float64"), ("f64b", "float64")):
            eng, U, mode, _, nugget = _prepared_engine(c, J, dtype=dtype, f32_start=True)
            trace = torch.empty((K_STEPS, c["p"], J), dtype=eng.torch_dtype, device=eng.device)
            eng.gp_run(mode, 3, K_STEPS, U, stride=1, trace=trace, nugget=nugget)
            _, _, per = eng.mh_stats(per_chain=True)
            out[key] = (trace.cpu().numpy(), U.cpu().numpy(), per.copy(), eng.mh_phi())
            eng.close()
        t32, u32, c32, _ = out["f32"]
        t64, u64, c64, p64 = out["f64"]
        assert t32.dtype == np.float32 and t64.dtype == np.float64
        assert np.array_equal(c32, c64) and 0 < c64.sum() < K_STEPS * J
        assert np.array_equal(t32, t64.astype(np.float32)) and np.array_equal(u32, u64.astype(np.float32))
        assert np.array_equal(t64[-1], u64)
        tb, ub, cb, pb = out["f64b"]
        assert np.array_equal(tb, t64) and np.array_equal(ub, u64) and np.array_equal(cb, c64) and np.array_equal(pb, p64)


def test_a_shard_draws_the_noise_of_its_global_columns():
    """An engine over the columns [33, 98) of J_global = 130 reproduces those columns of the whole-range fused run bit for
    bit (the Philox words carry j_offset + j; a chain's result depends neither on its tile nor on its lane)."""
    import torch
    lo, hi, Jg = 33, 98, 130
    c = dict(CASES[7], M=Jg)                                # gamma, p = 2, J_t = 33: three block rows of L^{-1}
    res = []
    for J, off, cols in ((Jg, 0, None), (hi - lo, lo, slice(lo, hi))):
        eng, U, mode, _, nugget = _prepared_engine(c, J, J_global=Jg, j_offset=off, cols=cols)
        trace = torch.empty((K_STEPS // 3, c["p"], J), dtype=eng.torch_dtype, device=eng.device)
        eng.gp_run(mode, 0, K_STEPS, U, stride=3, trace=trace, nugget=nugget)
        _, _, per = eng.mh_stats(per_chain=True)
        res.append((trace.cpu().numpy(), U.cpu().numpy(), per.copy(), eng.mh_phi()))
        eng.close()
    (tw, uw, cw, pw), (ts, us, cs, ps) = res
    assert np.array_equal(ts, tw[:, :, lo:hi]) and np.array_equal(us, uw[:, lo:hi])
    assert np.array_equal(cs, cw[lo:hi]) and np.array_equal(ps, pw[lo:hi]) and cw.sum() > 0


def test_start_on_training_points_without_the_nugget():
    """The construction of tests/test_gpu_gp.py::test_start_on_training_points with ``nugget=False``: the variance at a
    training point is zero up to rounding, of either sign, so phi of a start state may be NaN or inf.  No NaN enters U, and a
    chain whose phi is NaN stays where it started with counter 0."""
    from ces_amd import sample
    man, a = load_gold()
    enka = gold_problem(a)
    mc = sample.MCMC()
    mc.mute_bar, mc.y_obs, mc.noise = True, a["prob_y"], "device"
    mc.gp_mh(enka, 5, gold_prior(a), chains=30, start="ensemble", nugget=False, fused=True)
    assert mc.fused_launches == 1
    assert mc.samples.shape == (2, 6, 30) and np.array_equal(mc.samples[:, 0, :], enka.Ustar)
    assert np.all(np.isfinite(mc.samples))
    phi = mc._mh_eng.mh_phi()
    _, _, per = mc._mh_eng.mh_stats(per_chain=True)
    stuck = np.isnan(phi)
    assert np.all(per[stuck] == 0) and np.array_equal(mc.samples[:, -1, stuck], enka.Ustar[:, stuck])
    # the step path leaves the same chains
    ref = sample.MCMC()
    ref.mute_bar, ref.y_obs, ref.noise = True, a["prob_y"], "device"
    ref.gp_mh(enka, 5, gold_prior(a), chains=30, start="ensemble", nugget=False, fused=False)
    assert np.array_equal(np.isnan(ref._mh_eng.mh_phi()), stuck)
    assert np.array_equal(ref.accept_chains, mc.accept_chains)
    assert np.max(np.abs(ref.samples - mc.samples)) <= _bound(ref.samples, 5)


def test_errors():
    """cesx_gp_run before a start returns CESX_ESTATE; mode dense or proj, n_steps < 1 and a step index that reaches 2^31
    return CESX_EINVAL; an emulator beyond the LDS formula returns CESX_EUNSUPPORTED, which ``gp_mh(chains=, fused=True)``
    turns into ValueError.  Nothing is launched: the states are untouched, and the handle runs a valid launch afterwards."""
    import torch
    from ces_amd import emulate, engine as E, sample
    c = dict(CASES[16], M=8)                                # gamma with a diagonal Gamma, p = 2, four GPs
    enka, y, prior, kw = gc.problem(c)
    p, n, J = enka.p, enka.n_obs, 8
    eng = E.Engine(p, n, J, dtype="float64")
    U = eng.to_device(np.repeat(enka.Ustar.mean(axis=1)[:, None], J, axis=1), p, "U").clone()
    stream = eng._stream()

    def run(mode="gamma", step=0, n_steps=3):
        return eng.lib.cesx_gp_run(eng._h, E.GP_MODES[mode], step, n_steps, 1, 1, U.data_ptr(), None, None, None, stream)
    assert run() == E.ESTATE                                               # no problem at all
    eng.set_problem(y, kw["Gamma"], prior.mean, prior.cov, prior.mean)
    eng.mh_set_proposal(None, gc.scales_of(enka, kw))
    assert run() == E.ESTATE                                               # no emulator
    eng.gp_set(emulate.device_image(enka, enka.gpmodels))
    assert run() == E.ESTATE                                               # no start
    mean, _ = eng.gp_predict(U, var=False)
    eng.gp_start("gamma", U, mean)
    before = U.cpu().numpy().copy()
    assert run("dense") == E.EINVAL and b"step path" in eng.lib.cesx_last_error(eng._h)
    assert run("proj") == E.EINVAL and b"step path" in eng.lib.cesx_last_error(eng._h)
    assert run(n_steps=0) == E.EINVAL and run(step=2 ** 31 - 2) == E.EINVAL
    assert eng.lib.cesx_gp_run(eng._h, 0, 0, 3, 0, 1, U.data_ptr(), None, None, None, stream) == E.EINVAL      # stride < 1
    assert eng.lib.cesx_gp_run(eng._h, 0, 0, 3, 1, 1, None, None, None, None, stream) == E.EINVAL           # a null U
    with pytest.raises(ValueError):
        eng.gp_run("dense", 0, 3, U)
    torch.cuda.synchronize()
    assert np.array_equal(U.cpu().numpy(), before) and eng.mh_stats()[0] == 0
    assert run() == E.OK                                                   # the handle still runs a valid launch
    torch.cuda.synchronize()
    assert eng.mh_stats()[0] == 3 and np.all(np.isfinite(U.cpu().numpy()))

    # beyond the LDS formula: 256 (3 p + J_p + 2 n_gp) + 8192 > 160 KiB  <=>  J_p > 608 - 3 p - 2 n_gp.  Only the descriptor
    # is installed (zeros for L^{-1} and alpha: nothing is launched with it)
    Jt = 608 - 3 * p - 2 * n + 1
    img = dict(n=n, Jt=Jt, p=p, A=np.tile(np.eye(p), (n, 1, 1)), c=np.zeros(p), Z=np.zeros((n, Jt, p)),
               par=np.tile([1.0, 0.1, 0.0], (n, 1)), family=np.zeros(n, dtype=np.int32), mw=np.zeros((n, p)),
               alpha=np.zeros((n, Jt)), Li=np.tile(np.eye(Jt), (n, 1, 1)))
    eng.gp_set(img)
    before = U.cpu().numpy().copy()
    assert run() == E.EUNSUPPORTED and b"LDS" in eng.lib.cesx_last_error(eng._h)
    with pytest.raises(E.CesxError) as exc:
        eng.gp_run("gamma", 0, 3, U)
    assert exc.value.code == E.EUNSUPPORTED
    torch.cuda.synchronize()
    assert np.array_equal(U.cpu().numpy(), before) and eng.mh_stats()[0] == 3
    img_fit = dict(img, Jt=Jt - 16, Z=img["Z"][:, :Jt - 16], alpha=img["alpha"][:, :Jt - 16], Li=np.tile(np.eye(Jt - 16), (n, 1, 1)))
    eng.gp_set(img_fit)                                                    # the largest J_p that fits
    assert run() == E.OK
    torch.cuda.synchronize()
    assert eng.mh_stats()[0] == 6 and np.all(np.isfinite(U.cpu().numpy()))
    eng.close()

    # the driver: the same return as ValueError naming the LDS limit and fused=False
    rng = np.random.default_rng(0)
    big = random_gps(rng, 2, 1, 608, "RBF", lik=1e-2)
    mc = sample.MCMC()
    mc.mute_bar, mc.y_obs, mc.noise = True, np.zeros(1), "device"
    from scipy import stats
    with pytest.raises(ValueError, match="LDS.*fused=False"):
        mc.gp_mh(big, 2, stats.multivariate_normal(mean=np.zeros(2), cov=np.eye(2)), chains=2, fused=True, Gamma=np.eye(1))
    mc.gp_mh(big, 2, stats.multivariate_normal(mean=np.zeros(2), cov=np.eye(2)), chains=2, fused=False, Gamma=np.eye(1))
    assert mc.fused_launches == 0 and mc.samples.shape == (2, 3, 2)
