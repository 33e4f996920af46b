"""The streamed Darcy forward map on the device (cesx_darcy_set_streamed, ces_amd/csrc/kernels_darcy_stream.hip) against the
host map.

The yardstick everywhere is the host map ``ces_amd.darcy.model.__call__`` in fp64, particle by particle (for an fp32 engine
evaluated at the fp32-rounded inputs); the bound is tests/test_gpu_darcy.py's,

    max|g_dev - g_host| <= 16 cond_2(A) 2^-52 max|g_host|      (+ 2^-23 max|g_host| for the output rounding of an fp32 engine).

What the streamed form adds to go wrong -- a ring that wraps many times per particle, a workspace slot and the ring's LDS
reused by the next particle of a persistent workgroup, also behind an early exit on a bad pivot -- is held to bit equality
across grid sizes.  The largest observed ratio of a run and the streamed-resident difference are printed when the module's
tests are over (NOTEBOOK.md records them).
"""
import os
import sys

import numpy as np
import pytest
from scipy import stats

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import darcy_cases as dc  # noqa: E402
import darcy_stream_cases as sc  # noqa: E402

pytestmark = pytest.mark.gpu

WORST = {"ratio": 0.0, "case": None}
MUTUAL = {}


@pytest.fixture(scope="module")
def eng_mod():
    import torch
    from ces_amd import engine
    assert torch.cuda.is_available(), "these tests need the MI355X"
    yield engine
    print("\n[darcy-stream] worst |g_dev - g_host| / (cond_2(A) 2^-52 max|g_host|) over the fp64 cases of this run: %.3g at %s"
          % (WORST["ratio"], WORST["case"]))
    for k, v in MUTUAL.items():
        print("[darcy-stream] streamed against resident, %s: max |difference| / max|g| = %.3g" % (k, v))


def _slot_bytes(K):
    m = K - 2
    return m * m * (2 * m + 1) * 8


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("scale", sc.SCALES)
@pytest.mark.parametrize("shape", list(sc.SHAPES), ids=sc.SHAPE_IDS)
def test_map_against_the_host(eng_mod, shape, scale, dtype):
    import torch
    K, p, n_obs = shape
    J = sc.SHAPES[shape]
    ref = sc.reference(K, p, n_obs, scale, dtype)
    eng = eng_mod.Engine(p, n_obs, J, dtype=dtype)
    mdl = sc.make_model(K, p, n_obs)
    U = eng.to_device(np.array(ref["U"]), p, "U")
    G = mdl.forward_device(eng, U).cpu().numpy().astype(np.float64)
    assert G.shape == (n_obs, J) and np.all(np.isfinite(G))
    assert torch.count_nonzero(eng._darcy_status) == 0
    assert eng.darcy_workspace_bytes() % _slot_bytes(K) == 0 and 1 <= eng.darcy_workspace_bytes() // _slot_bytes(K) <= J
    sc.check(G, ref, dtype, (shape, scale, dtype), WORST)
    eng.close()


@pytest.mark.parametrize("shape", [(16, 256, 50), (5, 4, 3)], ids=lambda s: "K%d-p%d-n%d" % s)
def test_streamed_beside_resident(eng_mod, shape):
    """Where both kernels apply, both are within the bound of the host; their mutual difference is recorded, not asserted
    to be zero (the back substitutions sum in different orders)."""
    K, p, n_obs = shape
    J, scale = 32, 10
    ref = dc.reference(K, p, n_obs, scale, "float64")
    eng = eng_mod.Engine(p, n_obs, J, dtype="float64")
    U = eng.to_device(np.array(ref["U"][:, :J]), p, "U")
    out = {}
    for solver in ("resident", "streamed"):
        mdl = sc.make_model(K, p, n_obs, solver=solver)
        out[solver] = mdl.forward_device(eng, U).cpu().numpy()
        assert (eng.darcy_workspace_bytes() > 0) == (solver == "streamed")
        sc.check(out[solver], ref, "float64", (shape, solver), WORST if solver == "streamed" else None)
    gmax = np.max(np.abs(ref["G"][:, :J]), axis=0)
    MUTUAL["K%d-p%d-n%d" % shape] = float(np.max(np.max(np.abs(out["streamed"] - out["resident"]), axis=0) / gmax))
    eng.close()


def test_slot_reuse_is_invisible(eng_mod):
    """K = 17, J = 10, scale 10 (17 of its 32 reference particles pivot): with one and with three workgroups every workgroup
    solves several particles in the same ring and the same workspace slot.  G is bit-identical to the automatic grid's (one
    workgroup per particle here), two applies are bit-identical, and the workspace is slots n (2 m + 1) doubles."""
    import torch
    K, p, n_obs, J = 17, 20, 9, 10
    ref = sc.reference(K, p, n_obs, 10, "float64")
    assert np.sum(ref["amin"][:J] <= 0.0) >= 1
    eng = eng_mod.Engine(p, n_obs, J, dtype="float64")
    U = eng.to_device(np.array(ref["U"][:, :J]), p, "U")
    mdl = sc.make_model(K, p, n_obs)
    G0 = mdl.forward_device(eng, U).clone()
    assert eng.darcy_workspace_bytes() == J * _slot_bytes(K)          # (the automatic grid holds far more than 10)
    sc.check(G0.cpu().numpy(), ref, "float64", "slot reuse: automatic", WORST)
    for wgs in (1, 3):
        mdl.device_max_workgroups = wgs
        token = eng._darcy_token
        G1 = mdl.forward_device(eng, U).clone()
        assert eng._darcy_token is not token
        assert eng.darcy_workspace_bytes() == wgs * _slot_bytes(K)
        G2 = mdl.forward_device(eng, U).clone()
        assert torch.equal(G1, G0), wgs
        assert torch.equal(G2, G1), wgs
    eng.close()


class _ZeroBlockModel:
    """As tests/test_gpu_darcy.py's: S replaced by an integer matrix whose rows sum to zero, so that for xi = 0 the nodal field
    and with it A are exactly zero on the host and on the device alike.  K x K by repeating the difference pattern."""

    def device_descriptor(self, n_obs=None):
        d = super().device_descriptor(n_obs)
        K = d["K"]
        S = np.zeros((K, K))
        for i in range(K):
            S[i, i], S[i, (i + 1) % K] = 1.0, -1.0
        d["S"] = S
        return d


def _kl(desc, xi):
    K = desc["K"]
    Xi = np.zeros(K * K)
    Xi[desc["scatter"]] = xi
    L = desc["coef"] * Xi.reshape(K, K)
    L[0, 0] = 0.0
    return L


def test_singular_particle_in_the_middle_of_a_workgroups_sequence(eng_mod):
    """K = 17, J = 6, two workgroups: particle 2 is workgroup 0's second of three.  Its first pivot is an exact zero; the
    status word and the LinAlgError are the resident kernel's, its outputs NaN, and every other particle -- particle 4, which
    the same workgroup solves afterwards in the same ring and slot, included -- is within the bound of the same descriptor
    applied in numpy."""
    import torch
    from ces_amd import darcy

    class M(_ZeroBlockModel, darcy.model_trunc):
        pass
    K, p, n_obs, J, bad = 17, 20, 9, 6, 2
    mdl = M(Nmesh=float(K), p=p)
    mdl.obs_index = dc.make_model(K, p, n_obs).obs_index
    mdl.set_device_solver("streamed")
    mdl.device_max_workgroups = 2
    desc = mdl.device_descriptor(n_obs)
    rng = np.random.default_rng(5)
    Uh = rng.standard_normal((p, J))
    Uh[:, bad] = 0.0
    a = desc["S"] @ np.exp(desc["D"] @ _kl(desc, Uh[:, bad]) @ desc["D"].T) @ desc["S"].T
    assert np.all(a == 0.0) and np.all(darcy.assemble_gwf(a).toarray() == 0.0)
    with pytest.raises(np.linalg.LinAlgError):
        dc.apply_descriptor(desc, Uh[:, bad])
    eng = eng_mod.Engine(p, n_obs, J, dtype="float64")
    U = eng.to_device(Uh, p, "U")
    G = eng.empty(n_obs)
    with pytest.raises(np.linalg.LinAlgError, match=r"particle %d is singular \(zero pivot in column 0\)" % bad):
        mdl.forward_device(eng, U, out=G)
    torch.cuda.synchronize()
    assert eng.darcy_workspace_bytes() == 2 * _slot_bytes(K)
    st = eng._darcy_status.cpu().numpy()
    assert st[bad] == 1 and np.count_nonzero(st) == 1
    Gh = G.cpu().numpy()
    assert np.all(np.isnan(Gh[:, bad]))
    good = [j for j in range(J) if j != bad]
    want = np.stack([dc.apply_descriptor(desc, Uh[:, j]) for j in good], axis=1)
    cond = []
    for j in good:
        aj = desc["S"] @ np.exp(desc["D"] @ _kl(desc, Uh[:, j]) @ desc["D"].T) @ desc["S"].T
        cond.append(np.linalg.cond(darcy.assemble_gwf(aj).toarray()))
    sc.check(Gh[:, good], dict(G=want, cond=np.array(cond)), "float64", "singular: the other columns")
    eng.close()


def test_overflowing_particle_in_the_middle_of_a_workgroups_sequence(eng_mod):
    """The same placement with exp(theta) overflowing for particle 3 (workgroup 1's second of three): reported as NOT FINITE,
    outputs NaN, the others -- particle 5 behind it included -- within the bound of the host map."""
    import torch
    K, p, n_obs, J, bad = 17, 20, 9, 6, 3
    mdl = sc.make_model(K, p, n_obs)
    mdl.device_max_workgroups = 2
    rng = np.random.default_rng(2)
    Uh = rng.standard_normal((p, J))
    Uh[:, bad] = 1e5
    eng = eng_mod.Engine(p, n_obs, J, dtype="float64")
    G = eng.empty(n_obs)
    with pytest.raises(np.linalg.LinAlgError, match=r"particle %d is not finite \(NaN or inf in column" % bad):
        mdl.forward_device(eng, eng.to_device(Uh, p, "U"), out=G)
    torch.cuda.synchronize()
    st = eng._darcy_status.cpu().numpy()
    assert st[bad] < 0 and np.count_nonzero(st) == 1
    Gh = G.cpu().numpy()
    assert np.all(np.isnan(Gh[:, bad]))
    good = [j for j in range(J) if j != bad]
    sc.check(Gh[:, good], sc.host(mdl, Uh[:, good]), "float64", "overflow: the other columns", WORST)
    eng.close()


def test_reinstall_across_solvers(eng_mod):
    """One engine at K = 8: resident -> streamed -> resident.  Each apply runs the kernel of the installed map (the workspace
    exists only while the streamed one is installed), each is within the bound; another model installing its map forces a
    re-install, as in tests/test_gpu_darcy.py::test_reinstall."""
    K, p, n_obs, J = 8, 10, 12, 5
    eng = eng_mod.Engine(p, n_obs, J, dtype="float64")
    rng = np.random.default_rng(8)
    Uh = 3.0 * rng.standard_normal((p, J))
    U = eng.to_device(Uh, p, "U")
    mdl = sc.make_model(K, p, n_obs, solver=None)
    ref = sc.host(mdl, Uh)

    def check(m, r, case):
        G = m.forward_device(eng, U).cpu().numpy()
        sc.check(G, r, "float64", case, WORST if m.device_solver == "streamed" else None)
        return G
    out = []
    for solver, bytes_ in (("resident", 0), ("streamed", J * _slot_bytes(K)), ("resident", 0)):
        token = getattr(eng, "_darcy_token", None)
        mdl.set_device_solver(solver)
        out.append(check(mdl, ref, "reinstall: " + solver))
        assert eng._darcy_token is not token
        assert eng.darcy_workspace_bytes() == bytes_
    assert np.array_equal(out[0], out[2])
    other = sc.make_model(K, p, n_obs)
    other.tau = 2.0
    other.set_rank()
    other.obs_index = np.arange(n_obs)[::-1].copy()
    ref_other = sc.host(other, Uh)
    mdl.set_device_solver("streamed")
    for k in range(2):
        check(other, ref_other, "reinstall: other model %d" % k)
        token = eng._darcy_token
        check(mdl, ref, "reinstall: first model %d" % k)
        assert eng._darcy_token is not token
    token = eng._darcy_token
    mdl.forward_device(eng, U)
    assert eng._darcy_token is token                         # nothing changed: not installed again
    eng.close()


def _run_problem():
    K, p, n_obs = 17, 20, 9
    mdl = sc.make_model(K, p, n_obs)
    mdl.set_initial()
    rng = np.random.default_rng(12)
    gamma = 0.005
    Gamma = gamma ** 2 * np.identity(n_obs)
    y = mdl(mdl.ustar) + gamma * rng.standard_normal(n_obs)
    return mdl, rng, Gamma, y, (K, p, n_obs)


def test_device_resident_run(eng_mod):
    """``sampling.run`` with a streamed K = 17 model, J = 64, three iterations, device noise: the device loop ran (the hook is
    called once per iteration and once for the final ensemble), and every traced Gall[k] is the host map of Uall[k] within
    the bound."""
    from ces_amd.calibrate import sampling
    mdl, rng, Gamma, y, (K, p, n_obs) = _run_problem()
    J, T = 64, 3
    eks = sampling(p=p, n_obs=n_obs, J=J)
    eks.T, eks.ustar, eks.mu, eks.sigma = T, mdl.ustar.reshape(p, 1), np.zeros((p, 1)), 100.0 * np.identity(p)
    eks.noise = "device"
    assert eks._device_loop_ok(mdl, False, {})
    calls = []
    hook = mdl.forward_device
    mdl.forward_device = lambda *a, **k: (calls.append(1), hook(*a, **k))[1]
    eks.run(y, rng.standard_normal((p, J)), mdl, Gamma, np.linalg.cholesky(Gamma), t_tol=1e9)
    del mdl.forward_device
    assert len(calls) == T + 1
    assert eks.Uall.shape == (T + 1, p, J) and eks.Gall.shape == (T + 1, n_obs, J)
    assert np.all(np.isfinite(eks.Uall)) and np.all(np.isfinite(eks.Gall))
    dtype = str(eks.engine_dtype)
    for k in range(T + 1):
        sc.check(np.asarray(eks.Gall[k], dtype=np.float64), sc.host(mdl, np.asarray(eks.Uall[k], dtype=np.float64)), dtype,
                 "device-resident run, iterate %d" % k, WORST)


def test_sampler_many_chains(eng_mod):
    """``MCMC.model_mh(chains=8)`` with device noise and the streamed model: it runs, the samples are finite, the per-chain
    acceptance rates are rates, and the host map of the final states agrees with a fresh forward_device of them."""
    from ces_amd import calibrate, sample
    mdl, _, Gamma, y, (K, p, n_obs) = _run_problem()
    M = 8
    rng = np.random.default_rng(4)
    enka = calibrate.enka(p, n_obs, 130)
    enka.Ustar = mdl.ustar.reshape(p, 1) + 0.3 * rng.standard_normal((p, 130))
    mc = sample.MCMC()
    mc.mute_bar, mc.y_obs, mc.noise = True, y, "device"
    prior = stats.multivariate_normal(mean=np.zeros(p), cov=100.0 * np.identity(p))
    mc.model_mh(mdl, 10, prior, enka, Gamma, delta=1.0, chains=M, start="ensemble")
    assert mc.samples.shape == (p, 11, M) and np.all(np.isfinite(mc.samples))
    acc = np.asarray(mc.accept_chains)
    assert acc.shape == (M,) and np.all(acc >= 0.0) and np.all(acc <= 1.0)
    final = np.ascontiguousarray(mc.samples[:, -1, :])
    eng = eng_mod.Engine(p, n_obs, M, dtype="float64")
    G = mdl.forward_device(eng, eng.to_device(final, p, "U")).cpu().numpy()
    sc.check(G, sc.host(mdl, final), "float64", "model_mh: the final states", WORST)
    eng.close()
