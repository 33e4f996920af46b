"""The projected per-chain likelihood on the device (CESX_GP_PROJ, gp_score_proj_kernel; gp_mh(chains=, pca_tools=,
sigma_form='projected')).

The score is held ELEMENTWISE, through cesx_mh_phi: gp_start('proj') on crafted mean and variance rows (not through the GP),
then the chains' phi against the literal reference within the bound_j of tests/gp_proj_cases.py (the bar is in that module,
the measurement behind its constant in tests/gp_dense_cases.py).  The accept loop runs through run_accept_steps of
tests/test_gpu_sample_edges.py with the band max(1e-9 max(1, |phi|), bound(U) + bound(P)) and the cap of 1 chain-step in
1000 left out; guards around every buffer the kernel may write.

The literal reference factors an n x n matrix per chain on the host: at n = 300 and M = 257 it, not the device, is what a
case waits for (a few seconds).

Worst |phi - reference| / bound_j per part is printed (pytest -s) and recorded in NOTEBOOK.md."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gp_dense_cases as gc  # noqa: E402
import gp_proj_cases as gq  # noqa: E402
from edge_helpers import guarded, guards_intact, put, same_bits  # noqa: E402
from test_emulate_host import Enka, gold_prior, gold_problem, load_gold  # noqa: E402
from test_gpu_gp_dense import BETA, STEPS, VARIANTS, dense_engine, dev, host_chain, trivial_image  # noqa: E402
from test_gpu_sample_edges import SEED, eng_mod, note, run_accept_steps  # noqa: E402,F401

from oracle import stage_ref as sr  # noqa: E402

pytestmark = pytest.mark.gpu


def proj_engine(eng_mod, pr, M, dtype, kind, logdet, **kw):
    eng = eng_mod.Engine(pr["p"], pr["n"], M, dtype=dtype, **kw)
    eng.set_problem(pr["y"], pr["Gamma"], pr["mu"], pr["Sp"], pr["mu"])
    S = 0.3 * np.linalg.cholesky(pr["Sp"])
    eng.mh_set_proposal(kind, S, BETA)
    eng.gp_set(trivial_image(pr["p"], pr["k"]))
    eng.gp_proj_set(*gq.project(pr), logdet)
    return eng, S


def start_and_read(eng, U, Uh, m, v, mode="proj"):
    """gp_start(mode) on the rows, the chains' phi back; the states and the rows untouched."""
    put(U, Uh)
    md, vd = dev(eng, m), dev(eng, v)
    eng.gp_start(mode, U, md, vd)
    phi = eng.mh_phi()
    assert np.all(same_bits(U.cpu().numpy(), Uh))
    assert np.array_equal(md.cpu().numpy(), m) and np.array_equal(vd.cpu().numpy(), v, equal_nan=True)
    return phi


# ---- the score, elementwise ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("vi", range(len(VARIANTS)))
@pytest.mark.parametrize("n,k", gq.GPU_SHAPES)
def test_score_elementwise(eng_mod, n, k, vi):
    """(the variant table of tests/test_gpu_gp_dense.py: every shape meets every chain count, both log det values, both
    priors, both updates and both engine dtypes)"""
    assert {v[0] for v in VARIANTS} == set(gq.GPU_M)
    M, logdet, dense_prior, kind, dtype = VARIANTS[vi]
    rng = np.random.default_rng([n, k, vi])
    pr = gc.problem(rng, n, k, 1e4, "pca", dense_prior=dense_prior)
    eng, _ = proj_engine(eng_mod, pr, M, dtype, kind, logdet)
    U_flat, U = guarded(eng, pr["p"])
    Uh = gc.states(rng, pr, M, np.dtype(dtype))
    m, v = gc.rows(rng, k, M)
    phi = start_and_read(eng, U, Uh, m, v)
    want, bound, cond, _, cond_s = gq.reference(pr, m, v, Uh.astype(np.float64), logdet)
    assert np.all(cond_s <= gc.COND_SCORE), cond_s.max()
    ratio = float(np.max(np.abs(phi - want) / bound))
    w = note("proj score", ratio=ratio)
    print("gp_start proj %s n=%d k=%d M=%d logdet=%d %s prior %s: cond_2 up to %.1e, worst |phi - ref| / bound %.3g "
          "(so far %.3g)" % (dtype, n, k, M, logdet, "dense" if dense_prior else "diagonal", kind or "RW", cond.max(),
                             ratio, w["ratio"]))
    assert np.all(np.abs(phi - want) <= bound), (vi, ratio, np.flatnonzero(~(np.abs(phi - want) <= bound))[:8])
    assert guards_intact(U_flat, U)
    nsteps, rate, per = eng.mh_stats(per_chain=True)
    assert nsteps == 0 and rate == 0.0 and not per.any()


@pytest.mark.parametrize("n,k", [(50, 8), (64, 16), (128, 128)])
def test_the_same_answer_as_the_dense_mode(eng_mod, n, k):
    M = 70
    rng = np.random.default_rng([n, k, 21])
    pr = gc.problem(rng, n, k, 1e4, "pca", dense_prior=True)
    Uh = gc.states(rng, pr, M)
    m, v = gc.rows(rng, k, M)
    want, b_dense, _, _ = gc.reference(pr, m, v, Uh, True)
    _, b_proj, _, _, _ = gq.reference(pr, m, v, Uh, True)
    engd, _ = dense_engine(eng_mod, pr, M, "float64", None, True)
    _, Ud = guarded(engd, pr["p"])
    phi_d = start_and_read(engd, Ud, Uh, m, v, "dense")
    engp, _ = proj_engine(eng_mod, pr, M, "float64", None, True)
    _, Up = guarded(engp, pr["p"])
    phi_p = start_and_read(engp, Up, Uh, m, v)
    print("n=%d k=%d: dense %.3g, proj %.3g of their bounds; |dense - proj| %.3g of the sum"
          % (n, k, np.max(np.abs(phi_d - want) / b_dense), np.max(np.abs(phi_p - want) / b_proj),
             np.max(np.abs(phi_d - phi_p) / (b_dense + b_proj))))
    assert np.all(np.abs(phi_d - want) <= b_dense) and np.all(np.abs(phi_p - want) <= b_proj)
    assert np.all(np.abs(phi_d - phi_p) <= b_dense + b_proj)


# ---- the accept loop -----------------------------------------------------------------------------------------------------

def accept_case(eng_mod, n, k, M, dtype, kind, dense_prior, logdet, uniform=None, part="proj accept"):
    ndt = np.dtype(dtype)
    rng = np.random.default_rng([n, k, M, 1 if dtype == "float32" else 0, 1 if kind else 0, int(dense_prior), int(logdet)])
    pr = gc.problem(rng, n, k, 1e2, "pca", dense_prior=dense_prior, b_scale=(-2.0, 0.0))
    p = pr["p"]
    kw, step_ids = {}, list(range(STEPS))
    if uniform is not None:
        seed, j_offset, step_ids = uniform
        kw = dict(seed=seed, j_offset=j_offset, J_global=j_offset + M)
    eng, S = proj_engine(eng_mod, pr, M, dtype, kind, logdet, **kw)

    def ref_of(Xh, m, v):
        ph, b, cond, _, _ = gq.reference(pr, m, v, Xh.astype(np.float64), logdet)
        assert np.all(cond <= gc.COND_ACCEPT)
        return ph, b

    U_flat, U = guarded(eng, p)
    P_flat, P = guarded(eng, p)
    Uh = gc.states(rng, pr, M, ndt)
    m0, v0 = gc.rows(rng, k, M, v_lo=1e-6)
    phi_dev = start_and_read(eng, U, Uh, m0, v0)
    phi0, b0 = ref_of(Uh, m0, v0)
    assert np.all(np.abs(phi_dev - phi0) <= b0) and guards_intact(U_flat, U)
    ref = gc.DenseAcceptRef(phi0, b0)
    keep = [None, None]

    def make_step(i, Uh):
        Ph = sr.propose(Uh.astype(np.float64), S, rng.standard_normal((p, M)), kind, BETA).astype(ndt)
        m, v = gc.rows(rng, k, M, v_lo=1e-6)
        logu = np.log(rng.random(M)) if uniform is None else sr.log_uniform(M, seed, step_ids[i], j_offset)
        phi_p, b_p = ref_of(Ph, m, v)
        return dict(P=Ph, m=m, v=v, phi_p=phi_p, logu=logu, half_width=ref.half_width(b_p))

    def launch(step, d):
        put(P, d["P"])
        keep[:] = [dev(eng, d["m"]), dev(eng, d["v"])]
        lu = None if uniform is not None else dev(eng, d["logu"])
        eng.gp_accept("proj", step, U, P, keep[0], keep[1], logu=lu)
        assert np.all(same_bits(P.cpu().numpy(), d["P"]))

    label = "gp_accept proj %s n=%d k=%d M=%d %s %s prior logdet=%d%s" % (
        dtype, n, k, M, kind or "RW", "dense" if dense_prior else "diagonal", logdet,
        " device uniform j_offset=%d" % uniform[1] if uniform else "")
    Uh, taken = run_accept_steps(eng, U_flat, U, Uh, ref, step_ids, make_step, launch, label, part)
    assert guards_intact(P_flat, P)
    # the chains' phi after the loop: the reference's, within the bound of the state each chain holds
    phi_end = eng.mh_phi()
    assert np.all(np.abs(phi_end - ref.phi) <= ref.bound), float(np.max(np.abs(phi_end - ref.phi) / ref.bound))
    if M >= 33:
        assert 0 < taken < len(step_ids) * M, (label, taken)


# (the log det term where the chains are few: the reference's eigvals of an n x n matrix per chain-step is the cases' time)
ACCEPT_CASES = [(129, 4, 257, "float64", "pCN", True, False), (180, 16, 130, "float32", None, False, False),
                (180, 128, 33, "float64", None, False, True), (180, 128, 33, "float32", "pCN", True, True)]


@pytest.mark.parametrize("n,k,M,dtype,kind,dense_prior,logdet", ACCEPT_CASES)
def test_accept_loop(eng_mod, n, k, M, dtype, kind, dense_prior, logdet):
    accept_case(eng_mod, n, k, M, dtype, kind, dense_prior, logdet)


def test_accept_with_the_device_uniform(eng_mod):
    steps = [0, 1, 2, 3, 4, 5, 6, 2 ** 31 - 1]
    accept_case(eng_mod, 129, 4, 257, "float32", None, False, False, uniform=(SEED, 2 ** 32 + 7, steps), part="proj uniform")


# ---- an indefinite Sigma -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [4, 16, 33])
def test_an_indefinite_sigma_is_nan_rejects_and_leaves_its_wave_alone(eng_mod, k):
    """v = -10 in one chain of 257 (k = 4: chains 36 .. 39 share its wave; k = 16: 148 .. 151; k = 33: alone)."""
    n, M = 129, 257
    bad = {4: 37, 16: 150, 33: 64}[k]
    rng = np.random.default_rng([n, k, 13])
    pr = gc.problem(rng, n, k, 1e2, "pca", b_scale=(-2.0, 0.0))
    eng, S = proj_engine(eng_mod, pr, M, "float64", None, True)
    U_flat, U = guarded(eng, pr["p"])
    P_flat, P = guarded(eng, pr["p"])
    Uh = gc.states(rng, pr, M)
    m, v = gc.rows(rng, k, M, v_lo=1e-6)
    clean = start_and_read(eng, U, Uh, m, v)
    vb = v.copy()
    vb[1 % k, bad] = -10.0
    assert np.linalg.eigvalsh(gc.sigma_of(pr, vb[:, bad])).min() < 0.0
    phi = start_and_read(eng, U, Uh, m, vb)
    good = np.arange(M) != bad
    assert np.isnan(phi[bad]) and np.all(same_bits(phi[good], clean[good]))
    if k == 4:
        want, bound, _, _, _ = gq.reference(pr, m, vb, Uh, True)
        assert np.isnan(want[bad]) and np.all(np.abs(phi[good] - want[good]) <= bound[good])
    # the start state is stuck: a proposal any finite phi would take is refused
    Ph = sr.propose(Uh, S, rng.standard_normal((pr["p"], M)))
    put(P, Ph)
    m2, v2 = gc.rows(rng, k, M, v_lo=1e-6)
    lu = dev(eng, np.full(M, -1e6))
    eng.gp_accept("proj", 0, U, P, dev(eng, m2), dev(eng, v2), logu=lu)
    Un = U.cpu().numpy()
    assert np.all(same_bits(Un[:, bad], Uh[:, bad])) and np.all(same_bits(Un[:, good], Ph[:, good]))
    _, _, per = eng.mh_stats(per_chain=True)
    assert per[bad] == 0 and np.all(per[good] == 1)
    assert np.isnan(eng.mh_phi()[bad])
    # ... and an indefinite PROPOSAL is rejected by a chain with a finite phi
    clean = start_and_read(eng, U, Uh, m, v)
    put(P, Ph)
    v2b = v2.copy()
    v2b[0, bad] = -10.0
    assert np.linalg.eigvalsh(gc.sigma_of(pr, v2b[:, bad])).min() < 0.0
    eng.gp_accept("proj", 0, U, P, dev(eng, m2), dev(eng, v2b), logu=lu)
    Un = U.cpu().numpy()
    assert np.all(same_bits(Un[:, bad], Uh[:, bad])) and np.all(same_bits(Un[:, good], Ph[:, good]))
    after = eng.mh_phi()
    assert same_bits(after[[bad]], clean[[bad]])[0] and np.all(np.isfinite(after))
    assert guards_intact(U_flat, U) and guards_intact(P_flat, P)


# ---- determinism ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [3, 16, 33, 128])
def test_bits_do_not_depend_on_the_call_the_column_the_group_or_the_neighbours(eng_mod, k):
    n, M = 129, 257
    rng = np.random.default_rng([n, k, 9])
    pr = gc.problem(rng, n, k, 1e4, "pca", dense_prior=True)
    Uh = gc.states(rng, pr, M)
    m, v = gc.rows(rng, k, M)
    eng, _ = proj_engine(eng_mod, pr, M, "float64", None, True)
    _, U = guarded(eng, pr["p"])
    one = start_and_read(eng, U, Uh, m, v)
    two = start_and_read(eng, U, Uh, m, v)
    assert np.all(np.isfinite(one)) and np.all(same_bits(one, two))
    eng1, _ = proj_engine(eng_mod, pr, 1, "float64", None, True)
    _, U1 = guarded(eng1, pr["p"])
    for col in (0, 1, 2, 3, 64, 255, 256):                   # every group of a wave, a later wave, the ragged last wave
        alone = start_and_read(eng1, U1, Uh[:, [col]], m[:, [col]], v[:, [col]])
        assert same_bits(alone, one[[col]])[0], col
    # other neighbours, same bits
    m2, v2 = gc.rows(rng, k, M)
    m2[:, 65], v2[:, 65] = m[:, 2], v[:, 2]
    Uh2 = Uh.copy()
    Uh2[:, 65] = Uh[:, 2]
    three = start_and_read(eng, U, Uh2, m2, v2)
    assert same_bits(three[[65]], one[[2]])[0]


# ---- ABI states ----------------------------------------------------------------------------------------------------------

def test_abi_states(eng_mod):
    rng = np.random.default_rng(4)
    n, k, M = 7, 3, 5
    pr = gc.problem(rng, n, k, 1e2, "pca")
    R, a0, c_perp, hld = gq.project(pr)
    eng = eng_mod.Engine(pr["p"], n, M, dtype="float64")
    with pytest.raises(eng_mod.CesxError) as ei:                      # no problem yet
        eng.gp_proj_set(R, a0, c_perp, hld, True)
    assert ei.value.code == eng_mod.ESTATE and "cesx_set_problem" in str(ei.value)
    eng.set_problem(pr["y"], pr["Gamma"], pr["mu"], pr["Sp"], pr["mu"])
    eng.mh_set_proposal(None, 0.3 * np.linalg.cholesky(pr["Sp"]))
    eng.gp_set(trivial_image(pr["p"], k))
    _, U = guarded(eng, pr["p"])
    Uh = gc.states(rng, pr, M)
    put(U, Uh)
    m, v = gc.rows(rng, k, M)
    md, vd = dev(eng, m), dev(eng, v)
    with pytest.raises(eng_mod.CesxError) as ei:                      # no descriptor
        eng.gp_start("proj", U, md, vd)
    assert ei.value.code == eng_mod.ESTATE and "cesx_gp_proj_set" in str(ei.value)
    eng.gp_proj_set(R, a0, c_perp, hld, True)
    want, bound, _, _, _ = gq.reference(pr, m, v, Uh, True)
    eng.gp_start("proj", U, md, vd)
    assert np.all(np.abs(eng.mh_phi() - want) <= bound)
    Rnan, anan = R.copy(), a0.copy()
    Rnan[0, k - 1], anan[1] = np.inf, np.nan
    big = np.triu(np.ones((eng_mod.GP_PROJ_KMAX + 1,) * 2))
    refused = ((np.zeros((0, 0)), np.zeros(0), c_perp, hld, "k must be"), (big, np.ones(len(big)), c_perp, hld, "k must be"),
               (Rnan, a0, c_perp, hld, "non-finite"), (R, anan, c_perp, hld, "non-finite"), (R, a0, np.nan, hld, "non-finite"),
               (R, a0, c_perp, np.inf, "non-finite"), (R, a0, -1e-3, hld, "c_perp"))
    for args in refused:                                              # CESX_EINVAL: the installed descriptor stays
        with pytest.raises(ValueError, match=args[4]):
            eng.gp_proj_set(*args[:4], False)
    d = eng_mod.GpProjDesc(ctypes.sizeof(eng_mod.GpProjDesc), k, 0, None, a0.ctypes.data, c_perp, hld)      # a null R
    assert eng.lib.cesx_gp_proj_set(eng._h, ctypes.byref(d)) == eng_mod.EINVAL
    eng.gp_start("proj", U, md, vd)
    assert np.all(np.abs(eng.mh_phi() - want) <= bound)
    # below the diagonal nothing is read
    Rlow = R + np.tril(np.full((k, k), np.nan), -1)
    eng.gp_proj_set(Rlow, a0, c_perp, hld, True)
    eng.gp_start("proj", U, md, vd)
    assert np.all(np.abs(eng.mh_phi() - want) <= bound)
    eng.gp_set(trivial_image(pr["p"], n))
    with pytest.raises(ValueError, match="n_gp"):                     # the emulator's n_gp must be k (CESX_EINVAL)
        eng.gp_start("proj", U, md, vd)
    eng.gp_set(trivial_image(pr["p"], k))
    with pytest.raises(ValueError, match="null"):                     # the variance rows are needed
        eng.gp_start("proj", U, md, None)
    # a second problem drops the descriptor (and the proposal); (the binding passes only a CHANGED problem on)
    eng.set_problem(pr["y"] + 1.0, pr["Gamma"], pr["mu"], pr["Sp"], pr["mu"])
    eng.mh_set_proposal(None, 0.3 * np.linalg.cholesky(pr["Sp"]))
    with pytest.raises(eng_mod.CesxError) as ei:
        eng.gp_start("proj", U, md, vd)
    assert ei.value.code == eng_mod.ESTATE and "cesx_gp_proj_set" in str(ei.value)


# ---- end to end: gp_mh(chains=, pca_tools=, sigma_form='projected') -------------------------------------------------------

def stretched(a, n):
    """The golden problem's 4 GPs under a data space of n_obs = n: VD_k (n, 4) with orthogonal columns of mixed scales, a
    dense Gamma, and y where the emulator puts the ensemble mean, plus noise of Gamma's size."""
    enka = gold_problem(a)
    from ces_amd import emulate
    k = len(enka.gpmodels)
    rng = np.random.default_rng([n, 31])
    VD_k = np.linalg.qr(rng.standard_normal((n, k)))[0] * np.exp(rng.uniform(-1.0, 0.5, k))
    mG = rng.standard_normal((n, 1))
    A = rng.standard_normal((n, n)) / np.sqrt(n)
    Gamma = 0.02 * (0.5 * A @ A.T + 0.5 * np.eye(n))
    gm, _ = emulate.predict_gps(enka, enka.Ustar.mean(axis=1).reshape(1, -1))
    y = (VD_k @ gm + mG).reshape(n) + np.linalg.cholesky(Gamma) @ rng.standard_normal(n)
    big = Enka(enka.p, n, enka.Ustar, np.zeros((n, enka.Ustar.shape[1])))
    big.gpmodels = enka.gpmodels
    return big, y, Gamma, dict(VD_k=VD_k, mG=mG)


def _mc(y):
    from ces_amd import sample
    mc = sample.MCMC()
    mc.mute_bar = True
    mc.y_obs = y
    return mc


@pytest.mark.parametrize("n,compounded", [(129, False), (180, True)])
def test_chains1_reproduces_the_host_chain(n, compounded):
    man, a = load_gold()
    prior = gold_prior(a)
    enka, y, Gamma, pca = stretched(a, n)
    steps, seed = 20, 3200 + n
    kw = dict(pca_tools=pca, Gamma=Gamma, noise_compounded=compounded)

    def run(**extra):
        mc = _mc(y)
        np.random.seed(seed)
        mc.gp_mh(enka, steps, prior, **kw, **extra)
        return mc
    host = run()
    mine, margins, phis = host_chain(enka, prior, y, Gamma, pca, compounded, seed, steps)
    np.testing.assert_allclose(mine, host.samples, rtol=1e-12, atol=1e-12)       # the restatement IS the host chain
    d = run(chains=1, start="mean", sigma_form="projected")
    assert d.samples.shape == host.samples.shape == (enka.p, steps + 1)
    off = np.any(np.abs(d.samples - host.samples) > 1e-9 * np.maximum(1.0, np.abs(host.samples)), axis=0)
    if off.any():                      # a tie ends the comparison: the step before the first difference lay inside the band
        t = int(np.flatnonzero(off)[0]) - 1
        assert abs(margins[t]) <= sr.BAND * max(1.0, abs(phis[t])), (t, margins[t], phis[t])
    else:
        assert abs(d.accept - host.accept) < 1e-12
    assert 0.0 < host.accept < 1.0


def test_33_chains_run_and_keep_the_layout():
    man, a = load_gold()
    enka, y, Gamma, pca = stretched(a, 180)
    mc = _mc(y)
    mc.noise = "device"
    mc.trace_stride = 5
    mc.gp_mh(enka, 20, gold_prior(a), chains=33, pca_tools=pca, Gamma=Gamma, noise_compounded=True, sigma_form="projected")
    assert mc.samples.shape == (enka.p, 5, 33) and mc.accept_chains.shape == (33,)
    assert np.all(np.isfinite(mc.samples)) and 0.0 < mc.accept < 1.0
    assert abs(mc.accept - mc.accept_chains.mean()) < 1e-12


# ---- predict_gps(device=True, pca_tools=) ---------------------------------------------------------------------------------

def test_predict_gps_on_the_device_projects_back_on_the_host():
    """The k GPs on the device, the back-projection of ces/emulate.py:74-77 on the host: equal to the host path on one point,
    at the bar of the device prediction (tests/test_gpu_gp.py: 1e-9 of sum |alpha_j k_j| for a mean, of sigma^2 for a
    variance) carried through |VD_k|."""
    from ces_amd import emulate as em
    from test_gpu_gp import np_predict
    man, a = load_gold()
    enka, _, _, pca = stretched(a, 129)
    X = enka.Ustar[:, 3].reshape(1, -1) + 0.1
    V = np.abs(pca["VD_k"])
    for nugget in (True, False):
        hm, hv = em.predict_gps(enka, X, nugget=nugget, pca_tools=pca)
        dm, dv = em.predict_gps(enka, X, nugget=nugget, pca_tools=pca, device=True)
        assert dm.shape == hm.shape == (129, 1) and dv.shape == hv.shape == (129, 129)
        _, kv = em.predict_gps(enka, X, nugget=nugget)                   # the k GPs' own variances, on the host
        _, _, sc, s2 = np_predict(enka, enka.gpmodels, X, nugget)
        tol_m, tol_v = 1e-9 * sc, 1e-9 * s2 + 1e-9 * np.abs(kv).reshape(-1)
        assert np.all(np.abs(dm - hm) <= V @ tol_m + 1e-14 * np.abs(hm))    # (1e-14: the projection's own rounding)
        assert np.all(np.abs(dv - hv) <= (V * tol_v) @ V.T + 1e-14 * np.abs(hv))
    with pytest.raises(ValueError, match="separable"):
        em.predict_gps(enka, X, separable=True, device=True)
