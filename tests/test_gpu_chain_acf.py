"""The streaming lagged sums on the device (cesx_chain_acf_*, kernels_chainacf.hip; MCMC(..., chains=M, summary=True, autocorr=...)).

Engine level: synthetic traces (``ca.CASES``: ragged p, J and C < J, L at both ends, at the cap and on either side of the
sizes where the ring moves from 8 to 32 registers and on to LDS, N = L + 2, 2 L - 1 and 3 L + 5, a stuck chain and one at
10^6 x its spread) are uploaded in both engine dtypes and added in four chunkings.  Every output of the read is held
elementwise to  c 2^-52 B  against the extended-precision reference of the same, already rounded, trace
(tests/chain_acf_cases.py: the reference, the derivation of every c from the kernels' operation counts -- c_chain =
N + L + 8 per chain, c_red = ceil(C / 256) + 10 more for the pooled sums; tests/test_chain_acf_host.py shows the bounds see the
reference made wrong), and every output is the same bytes across the chunkings and across two identical runs.
Sampler level: the same run with and without ``autocorr=``, and ``self.autocorr`` against ``sample.autocorr_of_samples`` on
the trace of the same run without ``summary=``.  The two compute the same raw sums from the same draws, in fp64, in
different orders: each within (N + L + 8 + c_red) 2^-52 of sums of absolute values that are at most a few hundred times the
sums themselves here, so the finalised numbers agree to 1e-9 with eight digits to spare, unless a Geyer pair sits within
that of zero (it does not: the test would name the row).

Measured on an MI355X (worst ratio of |device - reference| to its bound over the engine-level table): NOTEBOOK.md,
"Autocorrelation ESS"."""
import os
import sys

import numpy as np
import pytest
from scipy import stats

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chain_acf_cases as ca  # noqa: E402
import chain_summary_cases as cs  # noqa: E402
import gp_chain_cases as gcc  # noqa: E402
import map_cases as mc_  # noqa: E402

pytestmark = pytest.mark.gpu
OUT = ("chain_gamma", "chain_mean", "gsum", "msum", "m2sum")


def _summed(eng, t, chunks, C, L):
    eng.chain_acf_begin(t.shape[0], L, C)
    a = 0
    for k in chunks:
        eng.chain_acf_add(t[a:a + k] if k > 1 else t[a])              # (a single draw as a (p, J) state: U_dev itself)
        a += k
    return eng.chain_acf_read(chains=True)


# ---- engine level -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("case", ca.CASES, ids=lambda c: "p%d-J%d-C%d-L%d-N%d" % c)
def test_raw_sums_against_extended_precision(case, dtype):
    import torch
    from ces_amd import engine, sample
    p, J, C, L, N = case
    x, ref, bounds = ca.case_ref(case, dtype)
    eng = engine.Engine(p, 2, J, dtype=dtype)
    t = torch.as_tensor(np.array(x), device=eng.device).to(eng.torch_dtype).contiguous()      # (a copy: the shared trace is read-only)
    assert np.array_equal(t.double().cpu().numpy(), x)                  # the upload is exact: the trace was rounded first
    outs = {name: _summed(eng, t, ch, C, L) for name, ch in ca.chunkings(N, L).items()}
    again = _summed(eng, t, [N], C, L)
    eng.close()
    one = outs["one"]
    worst = {k: ca.ratio(one[k], ref[k], bounds[k]) for k in OUT}
    print("\n[chain acf] %s %s LT=%d: worst |dev - ref| / bound %s" % (case, dtype, ca.lt_of(L), {k: "%.3g" % v for k, v in worst.items()}))
    assert all(v <= 1.0 for v in worst.values()), worst
    assert one["chain_gamma"].shape == (L + 1, p, C) and one["chain_mean"].shape == (p, C) and one["gsum"].shape == (p, L + 1)
    if J > 2 and C > 2:                                                 # the stuck chain: exact zeros, its mean its draw
        assert np.all(one["chain_gamma"][:, :, 2] == 0) and np.array_equal(one["chain_mean"][:, 2], x[0, :, 2])
    for name, out in outs.items():                                      # the cut into add calls changes no bit
        for k in OUT:
            assert out[k].tobytes() == one[k].tobytes(), (name, k)
    for k in OUT:                                                       # two identical runs: the same bits
        assert again[k].tobytes() == one[k].tobytes(), k
    # the estimator on the device's sums against the definition on the reference's
    fin = sample.finalise_autocorr(one, N, J, C, L)
    rho, tau, ess, trunc, W, vp = ca.estimator_ref(ref, N, J, C, L)
    ok = np.isfinite(vp) & (vp > 0)
    assert np.array_equal(np.isnan(fin["ess"]), ~ok | np.isnan(ess))
    assert np.allclose(fin["within"], W, rtol=1e-9, atol=0) and np.allclose(fin["var_plus"], vp, rtol=1e-9, atol=0)


def test_error_returns_leave_the_stage_alone():
    import torch
    from ces_amd import engine
    p, J, C, L, N = 3, 65, 64, 2, 11
    x, ref, bounds = ca.case_ref((p, J, C, L, N), "float64")
    eng = engine.Engine(p, 2, J, dtype="float64")
    t = torch.as_tensor(np.array(x), device=eng.device).contiguous()
    with pytest.raises(engine.CesxError) as exc:              # no begin yet
        eng.chain_acf_add(t[0])
    assert exc.value.code == engine.ESTATE and "has not been called" in str(exc.value)
    with pytest.raises(engine.CesxError) as exc:
        eng.chain_acf_read()
    assert exc.value.code == engine.ESTATE
    buf = np.empty(p * (L + 1))
    with pytest.raises(engine.CesxError) as exc:
        eng._check(eng.lib.cesx_chain_acf_read(eng._h, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, None, None, eng._stream()))
    assert exc.value.code == engine.ESTATE and "has not been called" in str(exc.value)
    clean = _summed(eng, t, [4, 7], C, L)
    # a run in hand, then every refused call in turn
    eng.chain_acf_begin(N, L, C)
    eng.chain_acf_add(t[:4])
    for args, match in (((N, 0, C), "lags must be"), ((N, ca.LAGS_MAX + 1, C), "lags must be"), ((N, L, 0), "n_chains must be"),
                        ((N, L, J + 1), "n_chains must be"), ((3, 1, C), "n_draws must be"), ((L + 1, L, C), "n_draws must be"),
                        ((ca.LAGS_MAX + 1, ca.LAGS_MAX, C), "n_draws must be")):
        with pytest.raises(ValueError, match=match):
            eng.chain_acf_begin(*args)
    with pytest.raises(ValueError, match="chain_acf_add: trace must be"):
        eng.chain_acf_add(t[:, :, :-1])
    with pytest.raises(ValueError, match="null pointer"):
        eng._check(eng.lib.cesx_chain_acf_add(eng._h, None, 1, eng._stream()))
    with pytest.raises(ValueError, match="kept must be"):
        eng._check(eng.lib.cesx_chain_acf_add(eng._h, t.data_ptr(), 0, eng._stream()))
    with pytest.raises(ValueError, match="null pointer"):
        eng._check(eng.lib.cesx_chain_acf_read(eng._h, None, buf.ctypes.data, buf.ctypes.data, None, None, eng._stream()))
    with pytest.raises(engine.CesxError) as exc:              # read before N draws
        eng.chain_acf_read()
    assert exc.value.code == engine.ESTATE and "fewer draws" in str(exc.value)
    with pytest.raises(engine.CesxError) as exc:              # add past N
        eng.chain_acf_add(t[:8])
    assert exc.value.code == engine.ESTATE and "more draws" in str(exc.value)
    eng.set_problem(np.zeros(2), np.eye(2), np.zeros(p), np.eye(p), np.zeros(p))      # a new problem does not touch the stage
    eng.chain_acf_add(t[4:])                                  # none launched anything: the run goes on as if never asked
    out = eng.chain_acf_read(chains=True)
    for k in OUT:
        assert out[k].tobytes() == clean[k].tobytes(), k
    again = eng.chain_acf_read(chains=True)                   # the stage stays readable
    for k in OUT:
        assert again[k].tobytes() == clean[k].tobytes(), k
    with pytest.raises(engine.CesxError) as exc:              # complete: one more draw is past N
        eng.chain_acf_add(t[0])
    assert exc.value.code == engine.ESTATE
    eng.close()
    sh = engine.Engine(p, 2, 32, dtype="float64", J_global=64)           # a shard of the chains
    with pytest.raises(ValueError, match="sharded"):
        sh.chain_acf_begin(N, L, 8)
    sh.close()


# ---- sampler level ----------------------------------------------------------------------------------------------------------

M, LAGS, FOLLOWED = 65, 7, 33


def _elliptic_sampler(stride=1):
    from ces_amd import calibrate, sample
    model, y, Gamma, mean, cov, _ = mc_.problem("elliptic", None)
    enka = calibrate.enka(2, 2, 130)
    enka.Ustar = mc_.start_ensemble("elliptic", 130, np.random.default_rng(4))
    s = sample.MCMC()
    s.mute_bar, s.y_obs, s.noise, s.trace_stride = True, y, "device", stride
    prior = stats.multivariate_normal(mean=mean, cov=cov)
    return s, lambda n, **kw: s.model_mh(model, n, prior, enka, Gamma, chains=M, start="ensemble", delta=0.7, **kw)


def _check_autocorr(ac, twin_samples, n_mcmc, stride, burn, chains=M, followed=FOLLOWED, lags=LAGS):
    """``ac`` against ``autocorr_of_samples`` on the first ``followed`` chains of the twin run's draws."""
    from ces_amd import sample
    draws = cs.draws_of(twin_samples, n_mcmc, stride, burn)               # (N, p, M)
    N = draws.shape[0]
    want = sample.autocorr_of_samples(draws[:, :, :followed].transpose(1, 0, 2), lags)
    assert ac["n"] == N == want["n"] and ac["chains"] == followed and ac["lags"] == lags
    assert ac["rho"].shape == (draws.shape[1], lags + 1) and ac["rho"].dtype == np.float64
    assert np.allclose(ac["rho"], want["rho"], rtol=1e-9, atol=1e-9, equal_nan=True)
    for k in ("tau", "within", "var_plus"):
        assert np.allclose(ac[k], want[k], rtol=1e-9, atol=0, equal_nan=True), k
    assert np.allclose(ac["ess"] * followed / chains, want["ess"], rtol=1e-9, atol=0, equal_nan=True)   # reported for all M chains
    assert np.array_equal(ac["truncated"], want["truncated"])
    assert np.all(ac["ess"] > 0) and np.all(ac["rho"][:, 0] == 1.0)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "steps"])
def test_model_mh_autocorr_equals_numpy_on_the_twins_trace(fused):
    import torch
    n = 40
    runs = []
    for extra in ({}, dict(summary=True), dict(summary=True, autocorr=dict(lags=LAGS, chains=FOLLOWED))):
        s, call = _elliptic_sampler()
        call(n, fused=fused, **extra)
        runs.append(s)
    tr, sm, ac = runs
    assert not hasattr(tr, "autocorr") and not hasattr(sm, "autocorr")
    assert torch.equal(sm.samples_device, ac.samples_device) and torch.equal(tr.samples_device, ac.samples_device)
    assert np.array_equal(sm.samples, ac.samples) and sm.accept == ac.accept and sm.fused_launches == ac.fused_launches
    assert (ac.fused_launches >= 1) == fused
    for k, v in sm.summary.items():                                       # the summary is the same bits with the kwarg
        assert np.array_equal(np.asarray(v), np.asarray(ac.summary[k])), k
    _check_autocorr(ac.autocorr, tr.samples, n, 1, 0)
    s, call = _elliptic_sampler()                                         # a later call without autocorr= removes the attribute
    call(n, fused=fused, summary=True, autocorr=3)
    assert s.autocorr["lags"] == 3 and s.autocorr["chains"] == M
    call(n, fused=fused, summary=True)
    assert not hasattr(s, "autocorr")


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "steps"])
def test_burn_and_stride(fused):
    n, stride, burn = 61, 3, 7                                            # draws after the steps 9, 12, .., 60: 18
    runs = []
    for extra in ({}, dict(summary=True, burn=burn, autocorr=dict(lags=LAGS, chains=FOLLOWED))):
        s, call = _elliptic_sampler(stride)
        call(n, fused=fused, **extra)
        runs.append(s)
    tr, ac = runs
    assert ac.autocorr["n"] == 18 == ac.summary["n"]
    _check_autocorr(ac.autocorr, tr.samples, n, stride, burn)


def test_gp_mh_autocorr():
    from ces_amd import sample
    c = gcc.cases()[1]                                                    # p = 2, 16 training points, one RBF GP, pCN
    n = 30
    runs = []
    for extra in ({}, dict(summary=True, autocorr=dict(lags=LAGS, chains=FOLLOWED))):
        enka, y, prior, kw = gcc.problem(c)
        s = sample.MCMC()
        s.mute_bar, s.y_obs, s.noise, s.seed = True, y, "device", gcc.SEED
        s.gp_mh(enka, n, prior, chains=M, **dict(kw, **extra))
        runs.append(s)
    tr, ac = runs
    assert np.array_equal(tr.samples[:, -1, :], ac.samples[:, -1, :]) and tr.accept == ac.accept
    _check_autocorr(ac.autocorr, tr.samples, n, 1, 0)


def test_adapt_with_burn():
    """``adapt=A`` with ``burn = A``: the draws are the states after the steps A + 1 .. n, at the frozen step."""
    n, A = 32, 8
    runs = []
    for extra in ({}, dict(summary=True, burn=A, autocorr=dict(lags=LAGS, chains=FOLLOWED))):
        s, call = _elliptic_sampler()
        call(n, update="hmc", leapfrog=2, adapt=A, **extra)
        runs.append(s)
    tr, ac = runs
    assert tr.adapt["multiplier"] == ac.adapt["multiplier"] and tr.accept == ac.accept
    assert ac.autocorr["n"] == n - A
    _check_autocorr(ac.autocorr, tr.samples, n, 1, A)
