"""The gradient samplers on the projected Sigma, without a GPU: MCMC.langevin_phi_grad_pca (the n-space restatement the device is
held to) against finite differences; the numpy restatement of gp_proj_coef_kernel (tests/gp_proj_grad_cases.py) against the
literal form within the bars, and its mutants outside them; the new symbols, the ABI version and what gp_mh refuses."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gp_dense_cases as gc  # noqa: E402
import gp_proj_cases as gq  # noqa: E402
import gp_proj_grad_cases as gg  # noqa: E402
from test_emulate_host import gold_prior, gold_problem, load_gold  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("cesx_gp_proj_coef", "cesx_gp_proj_langevin_start", "cesx_gp_proj_langevin_accept", "cesx_gp_proj_hmc_leap",
               "cesx_gp_proj_hmc_accept")


# ---- langevin_phi_grad_pca ------------------------------------------------------------------------------------------------

def smooth_emulator(rng, k, p):
    """k smooth rows on R^p with closed-form gradients: m_t = sin(W_t u + c_t), v_t = exp(V_t u - 2)."""
    W, c, V = rng.standard_normal((k, p)), rng.standard_normal(k), 0.5 * rng.standard_normal((k, p))

    def rows(u):                                             # u (N, p) -> mean, var (k, N), dmean, dvar (k, N, p)
        s = W @ u.T + c[:, None]
        mean, var = np.sin(s), np.exp(V @ u.T - 2.0)
        return mean, var, np.cos(s)[:, :, None] * W[:, None, :], var[:, :, None] * V[:, None, :]
    return rows


@pytest.mark.parametrize("logdet", [False, True])
@pytest.mark.parametrize("n,k", [(1, 1), (7, 3), (40, 8)])
def test_langevin_phi_grad_pca_is_the_gradient_of_its_own_phi(n, k, logdet):
    from ces_amd.sample import MCMC
    rng = np.random.default_rng([n, k, int(logdet)])
    pr = gc.problem(rng, n, k, 1e2 if n > 1 else 1, "pca", p=3, dense_prior=True)
    rows = smooth_emulator(rng, k, 3)
    u = pr["mu"][None, :] + 0.3 * rng.standard_normal((5, 3))

    def phi_grad(x):
        return MCMC.langevin_phi_grad_pca(*rows(x), x, pr["y"], pr["Gamma"], pr["B"], pr["g0"].reshape(-1, 1), logdet,
                                          pr["mu"], pr["Sp"])
    phi, grad = phi_grad(u)
    assert phi.shape == (5,) and grad.shape == (5, 3) and np.all(np.isfinite(phi)) and np.all(np.isfinite(grad))
    step = 1e-5
    for r in range(3):
        up, dn = u.copy(), u.copy()
        up[:, r] += step
        dn[:, r] -= step
        fd = (phi_grad(up)[0] - phi_grad(dn)[0]) / (2 * step)
        scale = np.maximum(1.0, np.abs(grad).max(axis=1))
        assert np.all(np.abs(fd - grad[:, r]) <= 1e-6 * scale), (r, np.abs(fd - grad[:, r]).max())
    # the data term is the literal reference's; an indefinite Sigma is NaN
    mean, var, dm, dv = rows(u)
    ref = gg.literal(pr, mean, var, logdet)
    pt, _ = gc.prior_term(pr, u.T)
    np.testing.assert_allclose(phi, ref["phi"] + pt, rtol=1e-10)
    var[0, 2] = -1e3
    bad, _ = MCMC.langevin_phi_grad_pca(mean, var, dm, dv, u, pr["y"], pr["Gamma"], pr["B"], pr["g0"], logdet, pr["mu"], pr["Sp"])
    assert np.isnan(bad[2]) and np.all(np.isfinite(np.delete(bad, 2)))


# ---- the restatement in the kernel's order against the literal form ------------------------------------------------------

HOST_CASES = [(n, k, gq.cond_gamma_of(n), (-2.0, 1.0), gc.COND_SCORE) for n, k in gq.HOST_SHAPES] + \
             [(gq.BIG_B[0], gq.BIG_B[1], 1e4, gq.BIG_B[2], None)]      # (B diag(v) B^T >> Gamma: exempt from the cap, as in gq)
CASE_IDS = ["n%d-k%d%s" % (c[0], c[1], "-bigB" if c[4] is None else "") for c in HOST_CASES]
WORST = {"phi": 0.0, "a": 0.0, "b": 0.0}


def _case(n, k, cg, b_scale, cap):
    return gg.coef_case(n, k, gq.HOST_M, cg, b_scale, 0, cap)


def test_the_case_tables_cover_what_they_must():
    assert (1, 1) in gq.HOST_SHAPES and (65, 65) in gq.HOST_SHAPES           # k = 1 and n = k
    assert len(gg.MUTANTS) >= 5 and len(gg.MEASURE_CASES) == len(gq.HOST_SHAPES) + 1
    assert (gg.C_E, gg.C_H) == (8.0, 16.0)


def test_the_literal_phi_is_gp_proj_cases_reference_without_its_prior_term():
    pr, m, v, ref = _case(*HOST_CASES[2])
    X = np.tile(pr["mu"][:, None], (1, gq.HOST_M))           # the prior term and its bar vanish at the prior mean
    for logdet in (False, True):
        phi, bound, cond, q, cond_s = gq.reference(pr, m, v, X, logdet)
        r = gg.take(ref, logdet)
        bar_phi = gg.bars(pr, r, logdet)[0]
        np.testing.assert_allclose(r["phi"], phi, rtol=1e-11)
        np.testing.assert_allclose(bar_phi, bound, rtol=1e-9)
        np.testing.assert_allclose(r["cond"], cond, rtol=1e-12)


@pytest.mark.parametrize("case", HOST_CASES, ids=CASE_IDS)
def test_the_kernels_order_stays_within_the_bars(case):
    pr, m, v, ref = _case(*case)
    proj = gq.project(pr)
    for logdet in (False, True):
        r = gg.take(ref, logdet)
        bar_phi, bar_e, _, bar_b = gg.bars(pr, r, logdet)
        ph, a, b = gg.kernel_order_proj_coef(pr, m, v, logdet, proj=proj)
        rp, ra, rb = (float(np.max(x)) for x in (np.abs(ph - r["phi"]) / bar_phi, np.abs(a - r["e"]) / bar_e,
                                                 np.abs(b - gg.coef_b(r["e"], r["h"], logdet)) / bar_b))
        for key, val in (("phi", rp), ("a", ra), ("b", rb)):
            WORST[key] = max(WORST[key], val)
        print("n=%d k=%d logdet=%d: worst ratios to the bars phi_data %.3g, a %.3g, b %.3g (so far %s)"
              % (case[0], case[1], logdet, rp, ra, rb, WORST))
        assert rp <= 1.0 and ra <= 1.0 and rb <= 1.0, (logdet, rp, ra, rb)
        if logdet:                                           # phi_data IS the score restatement's data term
            X = np.tile(pr["mu"][:, None], (1, m.shape[1]))
            assert np.array_equal(ph, gq.kernel_order_proj(pr, m, v, X, True, proj=proj))


@pytest.mark.parametrize("case", HOST_CASES, ids=CASE_IDS)
def test_every_mutant_leaves_four_bars(case):
    """(a NaN where the reference is finite has left the bar too)"""
    pr, m, v, ref = _case(*case)
    proj = gq.project(pr)
    shown = 0
    for logdet in (False, True):
        r = gg.take(ref, logdet)
        _, bar_e, _, bar_b = gg.bars(pr, r, logdet)
        rb = gg.coef_b(r["e"], r["h"], logdet)
        for mutant in gg.MUTANTS:
            if gg.mutant_is_identity(mutant, logdet):
                continue
            _, a, b = gg.kernel_order_proj_coef(pr, m, v, logdet, mutant=mutant, proj=proj)
            with np.errstate(invalid="ignore"):
                out = ~(np.abs(a - r["e"]) <= 4 * bar_e) | ~(np.abs(b - rb) <= 4 * bar_b)
            assert out.any(), (mutant, logdet)
            shown += 1
    assert shown == 2 * len(gg.MUTANTS) - 2


def test_an_indefinite_sigma_is_nan_in_the_restatement_and_the_reference():
    pr, m, v, _ = _case(*HOST_CASES[1])
    vb = np.array(v)
    vb[1, 3] = -10.0
    assert np.linalg.eigvalsh(gc.sigma_of(pr, vb[:, 3])).min() < 0.0
    ph, a, b = gg.kernel_order_proj_coef(pr, m, vb, True)
    ref = gg.literal(pr, m, vb, True)
    good = np.arange(m.shape[1]) != 3
    assert np.isnan(ph[3]) and np.all(np.isnan(a[:, 3])) and np.all(np.isnan(b[:, 3])) and np.isnan(ref["phi"][3])
    assert np.all(np.isfinite(ph[good])) and np.all(np.isfinite(a[:, good])) and np.all(np.isfinite(b[:, good]))


# ---- the accept loop's cap, on the CPU ------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", range(4))
def test_the_restatement_stays_within_the_accept_loops_cap(case):
    """tests/test_gpu_gp_proj_langevin.py's accept loop with the kernel-order restatement in the device's place, at its seeds:
    decisions against the literal reference outside the band, at most 1 chain-step in 1000 inside it.  (k = 128: the
    restatement's Python loops over 257 chains are the time, some ten seconds a case.)"""
    import test_gpu_gp_proj_langevin as dev_tests
    assert len(dev_tests.ACCEPT_CASES) == 4
    n, k, dtype, seed = dev_tests.ACCEPT_CASES[case]
    dev_tests.run_accept(None, n, k, 257, dtype, seed, device=False)


# ---- the ABI ----------------------------------------------------------------------------------------------------------------

def test_the_new_symbols_are_in_the_header_and_the_library_and_the_abi_version_stays():
    from ces_amd import build, engine
    hdr = open(os.path.join(ROOT, "include", "cesx.h")).read()
    assert "#define CESX_ABI_VERSION 10" in hdr and engine.ABI_VERSION == 10
    assert "kernels_gpprojgrad.hip" in build.SOURCES
    lib = engine.load_library()
    for name in NEW_SYMBOLS:
        assert "int %s(" % name in hdr and name in engine.EXPORTS and hasattr(lib, name), name
    assert lib.cesx_abi_version() == 10


# ---- what gp_mh takes and refuses ----------------------------------------------------------------------------------------

def test_pca_tools_takes_the_gradient_samplers_with_the_projected_form_alone():
    from ces_amd import emulate as em
    from ces_amd import sample
    man, a = load_gold()
    enka, prior = gold_problem(a), gold_prior(a)
    mc = sample.MCMC()
    mc.mute_bar, mc.y_obs = True, a["prob_y"]
    pca = dict(VD_k=a["prob_VD_k"], mG=a["prob_mG"])
    kw = dict(Gamma=a["prob_Gamma_dense"], pca_tools=pca)
    for update in ("langevin", "hmc"):
        for extra in ({}, dict(chains=4), dict(chains=4, sigma_form="dense"), dict(adapt=5), dict(chains=4, adapt=5)):
            with pytest.raises(ValueError, match="pca_tools") as exc:
                mc.gp_mh(enka, 20, prior, update=update, **kw, **extra)
            assert "sigma_form='projected'" in str(exc.value), extra
            if update == "hmc":
                assert "update='hmc'" in str(exc.value)
    with pytest.raises(ValueError, match="pca_tools") as exc:
        em.predict_gps(enka, enka.Ustar.T[:3], grad=True, pca_tools=pca)
    assert "sigma_form='projected'" in str(exc.value)
    # the projected form passes the refusals, a dense Gamma under noise_compounded included (the log det of Sigma is differentiated)
    for update in ("langevin", "hmc"):
        sample.MCMC._langevin_refusals(dict(update=update, chains=4, sigma_form="projected", noise_compounded=True, **kw), prior)
    # ... and what the projected form cannot do either stays refused before an engine is created
    with pytest.raises(ValueError, match="fused"):
        mc.gp_mh(enka, 20, prior, update="langevin", chains=4, sigma_form="projected", fused=True, **kw)
    with pytest.raises(ValueError, match="Matern12"):
        mc.gp_mh(gold_problem(a, family="Matern12"), 20, prior, update="hmc", chains=4, sigma_form="projected", **kw)
