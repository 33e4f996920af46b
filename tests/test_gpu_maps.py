"""The closed-form maps on the device (cesx_map_*, ces_amd/csrc/kernels_maps.hip) against the host classes of ces_amd.utils,
the resident ``sampling.run`` built on the hook, and the fused chain kernel (cesx_mh_run_map: K Metropolis steps per launch,
one chain per lane) against the step path (propose / forward_device / accept), the fp64 numpy phi and the host chain.
Cases, references and bounds: tests/map_cases.py."""
import ctypes
import os
import sys

import numpy as np
import pytest
from scipy import stats

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import rel_err  # noqa: E402
import map_cases as mc_  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = mc_.EPS
K_STEPS = 7


@pytest.fixture(scope="module")
def eng_mod():
    import torch
    from ces_amd import engine
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return engine


# ---- map apply -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("J", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("kind", ["elliptic", "banana"])
def test_map_against_the_host_class(eng_mod, kind, J, dtype):
    """|G_dev - G_host| <= 8 eps_T sum|terms| per entry (1 ulp for ocml's exp, the rounding of each operation, the store), the
    host class evaluated per column in fp64 at the values the engine holds.  An ``out=`` call is bit-identical, and a second
    model installed on the same engine in between is seen: the first one installs itself again."""
    from ces_amd import utils
    model = utils.elliptic() if kind == "elliptic" else utils.banana(a=1.3, b=0.4)
    other = utils.banana() if kind == "elliptic" else utils.elliptic()
    rng = np.random.default_rng(J)
    U = mc_.as_engine(mc_.draw_U(kind, J, rng), dtype)
    eng = eng_mod.Engine(2, 2, J, dtype=dtype)
    Ud = eng.to_device(U, 2, "U")
    want, bound = mc_.host_columns(model, U), 8 * EPS[dtype] * mc_.abs_terms(model, U)
    G = model.forward_device(eng, Ud).cpu().numpy().astype(np.float64)
    err = np.abs(G - want)
    print("\n[maps] %s J=%d %s: worst err / bound %.3g" % (kind, J, dtype, float(np.max(err / bound))))
    assert np.all(err <= bound)
    Go = other.forward_device(eng, Ud).cpu().numpy().astype(np.float64)
    assert np.all(np.abs(Go - mc_.host_columns(other, U)) <= 8 * EPS[dtype] * mc_.abs_terms(other, U))
    out = eng.empty(2)
    assert model.forward_device(eng, Ud, out=out) is out                 # (the re-install: the other model's map is gone)
    assert np.array_equal(out.cpu().numpy().astype(np.float64), G)
    if kind == "banana":                                                 # an edited parameter installs again too
        model.a = 2.0
        G2 = model.forward_device(eng, Ud).cpu().numpy().astype(np.float64)
        assert np.all(np.abs(G2 - mc_.host_columns(model, U)) <= 8 * EPS[dtype] * mc_.abs_terms(model, U))
    eng.close()


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("b", ["scalar", "vector", "zero"])
@pytest.mark.parametrize("shape", [(2, 2), (3, 5), (33, 17)], ids=lambda s: "p%d-n%d" % s)
def test_lineal_log_against_the_host_class(eng_mod, shape, b, dtype):
    """|G_dev - G_host| <= (p + 8) eps_T (|A| exp(U) + |b|): the dot-product bound gamma_{p+1} in any summation order, plus
    exp and the two stores.  Columns J in {1, 63, 64, 65, 257} on one problem per shape."""
    from ces_amd import utils
    p, n = shape
    rng = np.random.default_rng(p * 100 + n)
    A = rng.standard_normal((n, p))
    model = utils.lineal_log(A)
    model.b = {"scalar": 0.75, "vector": rng.standard_normal(n), "zero": 0}[b]
    for J in (1, 63, 64, 65, 257):
        U = mc_.as_engine(rng.normal(0.0, 1.0, (p, J)), dtype)
        eng = eng_mod.Engine(p, n, J, dtype=dtype)
        Ud = eng.to_device(U, p, "U")
        want = np.stack([model(U[:, j]) for j in range(J)], axis=1)
        bound = (p + 8) * EPS[dtype] * (np.abs(A) @ np.exp(U) + np.abs(np.broadcast_to(np.asarray(model.b, dtype=np.float64), (n,)))[:, None])
        G = model.forward_device(eng, Ud).cpu().numpy().astype(np.float64)
        err = np.abs(G - want)
        print("\n[maps] lineal_log p=%d n=%d J=%d b=%s %s: worst err / bound %.3g" % (p, n, J, b, dtype, float(np.max(err / bound))))
        assert np.all(err <= bound), (J, float(np.max(err / bound)))
        assert np.array_equal(Ud.cpu().numpy().astype(np.float64), U)    # exp went to the scratch buffer, not over U
        out = eng.empty(n)
        assert model.forward_device(eng, Ud, out=out) is out
        assert np.array_equal(out.cpu().numpy().astype(np.float64), G)
        eng.close()


# ---- resident sampling.run ----------------------------------------------------------------------------------------------

def test_device_resident_run(eng_mod):
    """``sampling.run`` with an elliptic ensemble (J = 64, T = 3, device noise): the device loop is taken, and it equals the
    plain loop (the host map through G_ens, the same device noise) to the tolerance tests/test_gpu_darcy.py uses for that
    comparison: Uall and Gall to 1e-9 relative, metrics['t'] to 1e-8."""
    from ces_amd import utils
    from ces_amd.calibrate import sampling
    J, T, p, n = 64, 3, 2, 2
    rng = np.random.default_rng(1)
    U0 = np.vstack([rng.normal(0.0, 1.5, J), rng.uniform(90.0, 110.0, J)])
    runs = []
    for device_loop in (True, False):
        mdl = utils.elliptic()
        eks = sampling(p=p, n_obs=n, J=J)
        eks.T, eks.ustar, eks.mu, eks.sigma = T, np.array([[-2.65], [104.5]]), np.zeros((p, 1)), 100.0 * np.identity(p)
        eks.noise, eks.device_loop = "device", device_loop
        assert bool(eks._device_loop_ok(mdl, False, {})) == device_loop
        eks.run(mc_.ELLIPTIC_Y, np.copy(U0), mdl, mc_.ELLIPTIC_GAMMA, np.linalg.cholesky(mc_.ELLIPTIC_GAMMA), t_tol=1e9)
        runs.append(eks)
    dev, host = runs
    assert getattr(dev, "Ustar_device", None) is not None and tuple(dev.Ustar_device.shape) == (p, J)
    assert dev.Uall.shape == host.Uall.shape == (T + 1, p, J) and dev.Gall.shape == host.Gall.shape == (T + 1, n, J)
    eu, eg = rel_err(dev.Uall, host.Uall), rel_err(dev.Gall, host.Gall)
    print("\n[maps] device-resident elliptic run: rel err Uall %.3g Gall %.3g" % (eu, eg))
    assert eu < 1e-9 and eg < 1e-9
    assert len(dev.metrics["t"]) == T and np.allclose(dev.metrics["t"], host.metrics["t"], rtol=1e-8, atol=0.0)


# ---- fused against the step path -----------------------------------------------------------------------------------------

_ENGINES = {}


def _sampler(kind, update, M, noise="device", dtype="float64", stride=1):
    """An MCMC object, its enka (130 particles near the posterior's bulk) and the prior; samplers of one (M, dtype) share one
    engine, so a fused run follows a step-path run on the same handle."""
    from ces_amd import calibrate, sample
    prob = mc_.problem(kind, update)
    model, y, Gamma, mean, cov, _ = prob
    enka = calibrate.enka(2, 2, 130)
    enka.Ustar = mc_.start_ensemble(kind, 130, np.random.default_rng(4))
    s = sample.MCMC()
    s.mute_bar, s.y_obs, s.noise, s.engine_dtype, s.trace_stride = True, y, noise, dtype, stride
    key = (2, 2, M, dtype, int(s.device), int(s.seed))
    if key not in _ENGINES:
        _ENGINES[key] = s._mh_engine(2, 2, M)
    s._mh_eng, s._mh_key = _ENGINES[key], key
    return s, enka, stats.multivariate_normal(mean=mean, cov=cov), prob


def _run(kind, update, M, fused, n_mcmc, stride, start_step=0, noise="device", seed=None):
    s, enka, prior, prob = _sampler(kind, update, M, noise=noise, stride=stride)
    kw = dict(chains=M, start="ensemble", delta=0.7)
    if update is not None:
        kw.update(update=update, beta=mc_.BETA[kind])
    if seed is not None:
        np.random.seed(seed)
    if start_step:                                         # the resume path: the first leg on the step path for both
        s.model_mh(prob[0], start_step, prior, enka, prob[2], fused=False, **kw)
        assert s._mh_next_step == start_step
    first = 0 if not start_step else s.samples.shape[1]
    s.model_mh(prob[0], n_mcmc, prior, enka, prob[2], fused=fused, **kw)
    samples = s.samples.reshape(2, s.samples.shape[1], M)
    return s, samples[:, first:, :], np.rint(np.asarray(s.accept_chains) * n_mcmc).astype(np.int64), prob


def _bound(samples):
    return 4 * K_STEPS * 2.0 ** -52 * max(1.0, float(np.max(np.abs(samples))))


CONFIGS = [("elliptic", None), ("elliptic", "pCN"), ("banana", None), ("banana", "pCN")]


@pytest.mark.parametrize("M", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("kind, update", CONFIGS, ids=["%s-%s" % (k, u or "RW") for k, u in CONFIGS])
def test_fused_equals_the_step_path(eng_mod, kind, update, M):
    """Same seed, device noise, K = 7 steps, stride 1 and 3, from step 0 and from step 5 through the resume path: the
    per-chain accept counters are equal (no chain excluded: a flipped decision needs log u within rounding of phi(U) -
    phi(P), probability of order M K 1e-15), the kept samples have the same shape and agree within 4 K 2^-52 max(1, max|U|)
    (two ulp per proposal for the differing product order, accumulated over K steps).  The random walk runs with a dense
    prior covariance, elliptic with its diagonal Gamma, banana with its dense one.  mh_phi() after the fused run is the fp64
    numpy phi of the final states within 32 2^-52 sum|terms|."""
    for stride in (1, 3):
        for start_step in (0, 5):
            _, a, ca, _ = _run(kind, update, M, False, K_STEPS, stride, start_step)
            s, b, cb, prob = _run(kind, update, M, True, K_STEPS, stride, start_step)
            case = (stride, start_step)
            assert a.shape == b.shape == (2, (0 if start_step else 1) + K_STEPS // stride + (1 if K_STEPS % stride else 0), M), case
            assert np.array_equal(ca, cb), case
            if stride == 1 and start_step == 0 and M >= 63:
                assert 0 < ca.sum() < K_STEPS * M                 # proposals are accepted and rejected alike
            err = float(np.max(np.abs(a - b)))
            print("\n[maps] fused vs step %s %s M=%d stride=%d start=%d: max err %.3g (bound %.3g), accepted %d of %d"
                  % (kind, update or "RW", M, stride, start_step, err, _bound(a), ca.sum(), K_STEPS * M))
            assert err <= _bound(a), case
            final = np.ascontiguousarray(b[:, -1, :])
            assert np.array_equal(s.samples_device.cpu().numpy(), final)
            phi, mag = mc_.phi_numpy(prob, final)
            got = s._mh_eng.mh_phi()
            assert np.all(np.abs(got - phi) <= 32 * 2.0 ** -52 * mag), (case, float(np.max(np.abs(got - phi) / mag)))
            steps, _, per = s._mh_eng.mh_stats(per_chain=True)
            assert steps == K_STEPS and np.array_equal(per.astype(np.int64), cb)


def _prepared_engine(eng_mod, kind, update, J, dtype="float64", J_global=None, j_offset=0, cols=None):
    """An engine with the problem, the proposal, the model's map and the start states scored: (eng, model, U, prob)."""
    prob = mc_.problem(kind, update)
    model, y, Gamma, mean, cov, _ = prob
    eng = eng_mod.Engine(2, 2, J, dtype=dtype, J_global=J_global, j_offset=j_offset, seed=77)
    eng.set_problem(y, Gamma, mean, cov, mean)
    S = 0.7 * np.linalg.cholesky(np.cov(mc_.start_ensemble(kind, 130, np.random.default_rng(4))))
    eng.mh_set_proposal(update, np.linalg.cholesky(cov) if update == "pCN" else S, mc_.BETA[kind])
    U0 = mc_.start_ensemble(kind, J_global or J, np.random.default_rng(9)).astype(np.float32).astype(np.float64)
    if cols is not None:
        U0 = np.ascontiguousarray(U0[:, cols])
    U = eng.to_device(U0, 2, "U0").clone()
    eng.mh_start(U, model.forward_device(eng, U))
    return eng, model, U, prob


def test_fused_launches_and_single_steps_alternate(eng_mod):
    """A 4-step fused launch, one single step through propose / forward_device / accept, 2 more fused steps: equal to 7
    single steps under the bound of the fused comparison, with equal counters; mh_stats reports 7 steps."""
    import torch
    J = 65
    ends = []
    for mixed in (False, True):
        eng, model, U, _ = _prepared_engine(eng_mod, "elliptic", None, J)
        P, GP = eng.empty(2), eng.empty(2)

        def single(step):
            eng.mh_propose(step, U, out=P)
            model.forward_device(eng, P, out=GP)
            eng.mh_accept(step, U, P, GP)
        if mixed:
            eng.mh_run_map(0, 4, U)
            single(4)
            eng.mh_run_map(5, 2, U)
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
    assert np.max(np.abs(Ua - Ub)) <= _bound(Ua)
    assert np.allclose(pa, pb, rtol=0.0, atol=1e-9)


@pytest.mark.parametrize("M", [1, 65])
def test_fused_with_injected_noise(eng_mod, M):
    """``noise='numpy'`` under one np.random.seed: fused=True equals fused=False under the bound of the fused comparison (the
    draws are stacked per launch in the step loop's order), the samples have shape (p, n_mcmc + 1, M); for M = 1 it is also
    the host ``model_mh`` without ``chains=`` under the same seed (elliptic, random walk and pCN)."""
    from ces_amd import sample
    n_mcmc = K_STEPS
    for kind, update in (("elliptic", None), ("banana", "pCN")):
        _, a, ca, _ = _run(kind, update, M, False, n_mcmc, 1, noise="numpy", seed=11)
        s, b, cb, prob = _run(kind, update, M, True, n_mcmc, 1, noise="numpy", seed=11)
        assert s.samples.shape == ((2, n_mcmc + 1) if M == 1 else (2, n_mcmc + 1, M))
        assert np.array_equal(ca, cb) and np.max(np.abs(a - b)) <= _bound(a)
    if M == 1:
        # (elliptic only: the host banana class draws two normals from the global RNG in every call, noise or not -- the
        #  reference's quirk, tests/test_maps_host.py -- so a host banana chain consumes draws no device chain sees)
        for kind, update in (("elliptic", None), ("elliptic", "pCN")):
            kw = {} if update is None else dict(update=update, beta=mc_.BETA[kind])
            s, enka, prior, prob = _sampler(kind, update, 1, noise="numpy")
            np.random.seed(5)
            s.model_mh(prob[0], n_mcmc, prior, enka, prob[2], delta=0.7, chains=1, fused=True, **kw)
            host = sample.MCMC()
            host.mute_bar, host.y_obs = True, prob[1]
            np.random.seed(5)
            host.model_mh(prob[0], n_mcmc, prior, enka, prob[2], delta=0.7, **kw)
            assert s.samples.shape == host.samples.shape == (2, n_mcmc + 1)
            assert np.max(np.abs(s.samples - host.samples)) <= _bound(host.samples)
            assert s.accept == pytest.approx(host.accept, abs=1e-12)


def test_fp32_engine_is_the_fp64_launch_rounded_on_the_store(eng_mod):
    """One fused launch (K = 7, device noise, the same seed) on an fp32 and on an fp64 engine from start states exactly
    representable in fp32: within a launch all arithmetic is fp64 and both engines draw the same normals, so the fp32 trace
    is the fp64 trace cast to float32 bit for bit and the counters are equal."""
    import torch
    J = 65
    for kind, update in (("elliptic", None), ("banana", "pCN")):
        out = {}
        for dtype in ("float32", "float64"):
            eng, model, U, _ = _prepared_engine(eng_mod, kind, update, J, dtype=dtype)
            trace = torch.empty((K_STEPS, 2, J), dtype=eng.torch_dtype, device=eng.device)
            eng.mh_run_map(3, K_STEPS, U, stride=1, trace=trace)
            _, _, per = eng.mh_stats(per_chain=True)
            out[dtype] = (trace.cpu().numpy(), U.cpu().numpy(), per.copy())
            eng.close()
        t32, u32, c32 = out["float32"]
        t64, u64, c64 = out["float64"]
        assert t32.dtype == np.float32 and t64.dtype == np.float64
        assert np.array_equal(c32, c64) and 0 < c64.sum() < K_STEPS * J
        assert np.array_equal(t32, t64.astype(np.float32)) and np.array_equal(u32, u64.astype(np.float32))
        assert np.array_equal(t64[-1], u64)


def test_a_shard_draws_the_noise_of_its_global_columns(eng_mod):
    """An engine over the columns [33, 98) of J_global = 130 reproduces those columns of the whole-range fused run bit for
    bit (the Philox words carry j_offset + j)."""
    import torch
    lo, hi, Jg = 33, 98, 130
    res = []
    for J, off, cols in ((Jg, 0, None), (hi - lo, lo, slice(lo, hi))):
        eng, model, U, _ = _prepared_engine(eng_mod, "banana", None, J, J_global=Jg, j_offset=off, cols=cols)
        trace = torch.empty((K_STEPS // 3, 2, J), dtype=eng.torch_dtype, device=eng.device)
        eng.mh_run_map(0, K_STEPS, U, stride=3, trace=trace)
        _, _, per = eng.mh_stats(per_chain=True)
        res.append((trace.cpu().numpy(), U.cpu().numpy(), per.copy(), eng.mh_phi()))
        eng.close()
    (tw, uw, cw, pw), (ts, us, cs, ps) = res
    assert np.array_equal(ts, tw[:, :, lo:hi]) and np.array_equal(us, uw[:, lo:hi])
    assert np.array_equal(cs, cw[lo:hi]) and np.array_equal(ps, pw[lo:hi]) and cw.sum() > 0


def test_errors(eng_mod):
    """cesx_mh_run_map before cesx_mh_start, or with no fused map installed, returns CESX_ESTATE; cesx_map_set(ELLIPTIC) on an
    engine with p = 3 returns CESX_EINVAL; the states are untouched."""
    from ces_amd import utils
    E = eng_mod
    prob = mc_.problem("elliptic", None)
    model, y, Gamma, mean, cov, _ = prob
    J = 8
    eng = E.Engine(2, 2, J, dtype="float64")
    U0 = mc_.start_ensemble("elliptic", J, np.random.default_rng(0))
    U = eng.to_device(U0, 2, "U").clone()
    stream = eng._stream()

    def run_map():
        return eng.lib.cesx_mh_run_map(eng._h, 0, 3, 1, U.data_ptr(), None, None, None, stream)
    assert run_map() == E.ESTATE                                            # no problem at all
    eng.set_problem(y, Gamma, mean, cov, mean)
    eng.mh_set_proposal(None, 0.1 * np.identity(2))
    model.ensure_installed(eng)
    assert run_map() == E.ESTATE                                            # a proposal and a fused map, but no mh_start
    G = model.forward_device(eng, U)
    eng.mh_start(U, G)
    assert run_map() == E.OK
    with pytest.raises(ValueError):
        eng.mh_run_map(0, 0, U)                                             # n_steps < 1: CESX_EINVAL
    assert eng.lib.cesx_mh_run_map(eng._h, 2 ** 31 - 2, 3, 1, U.data_ptr(), None, None, None, stream) == E.EINVAL
    eng.map_set("exp")                                                      # installed, but no fused kind
    assert run_map() == E.ESTATE
    with pytest.raises(E.CesxError) as exc:
        eng.mh_run_map(0, 3, U)
    assert exc.value.code == E.ESTATE
    before = U.cpu().numpy().copy()
    assert run_map() == E.ESTATE and np.array_equal(U.cpu().numpy(), before)
    eng.close()
    # no map at all on a fresh handle: apply is a state error too
    eng = E.Engine(2, 2, J, dtype="float64")
    V = eng.empty(2)
    assert eng.lib.cesx_map_apply(eng._h, V.data_ptr(), eng.empty(2).data_ptr(), eng._stream()) == E.ESTATE
    eng.close()
    eng3 = E.Engine(3, 2, J, dtype="float64")
    d = E.MapDesc()
    d.struct_bytes = ctypes.sizeof(E.MapDesc)
    for kind in ("elliptic", "banana"):
        d.kind = E.MAP_KINDS[kind]
        d.prm[0], d.prm[1] = 0.25, 0.75
        assert eng3.lib.cesx_map_set(eng3._h, ctypes.byref(d)) == E.EINVAL
    with pytest.raises(ValueError, match="p = n_obs = 2"):
        utils.elliptic().ensure_installed(eng3)
    d.kind = E.MAP_KINDS["exp"]
    assert eng3.lib.cesx_map_set(eng3._h, ctypes.byref(d)) == E.OK
    d.kind = 9
    assert eng3.lib.cesx_map_set(eng3._h, ctypes.byref(d)) == E.EINVAL
    eng3.close()
