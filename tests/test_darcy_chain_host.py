"""Darcy chains on the adjoint launch, no GPU: the ABI's addition (cesx_mh_grad_source; still version 10, no new chain-taking entry
point), what ``model_mh(chains=M, update='langevin' / 'hmc')`` refuses before an engine exists, the numpy restatement of the
READY score (tests/darcy_chain_cases.py) against the host chain's yardsticks (darcy_grad_cases.host_score / np_step), and the
choice of the injected blocks of the GPU tests."""
import os
import sys

import numpy as np
import pytest
from scipy import stats

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import darcy_chain_cases as cc  # noqa: E402
import darcy_grad_cases as gc  # noqa: E402
import sampler_reuse_cases as sc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_10_with_the_install_call_and_no_new_chain_entry_point():
    from ces_amd import build, engine
    with open(os.path.join(ROOT, "include", "cesx.h")) as fh:
        hdr = fh.read()
    assert "#define CESX_ABI_VERSION 10" in hdr and engine.ABI_VERSION == 10
    assert "int cesx_mh_grad_source(cesx_handle h, int source);" in hdr
    assert "#define CESX_MH_GRAD_JACOBIAN 0" in hdr and "#define CESX_MH_GRAD_READY    1" in hdr
    assert "cesx_mh_grad_source" in engine.EXPORTS and engine.GRAD_SOURCES == {"jacobian": 0, "ready": 1}
    assert "kernels_darcy_chain.hip" in build.SOURCES
    lib = engine.load_library()
    assert lib.cesx_abi_version() == 10 and hasattr(lib, "cesx_mh_grad_source")
    # the call takes no chains: it is no column of the call-order table, and the table is as it was
    names = sc.chain_entry_points()
    assert names == sorted(sc.COLUMNS) and "cesx_mh_grad_source" not in names
    assert "cesx_mh_grad_source" in sc.header_entry_points()


def _sampler(gkind="diag"):
    from ces_amd import calibrate, sample
    prob = gc.step_problem(gkind)
    K, p, n = gc.STEP_SHAPE
    enka = calibrate.enka(p, n, gc.M_STEP)
    enka.Ustar = np.array(prob["Ustar"])
    s = sample.MCMC()
    s.mute_bar, s.y_obs = True, prob["y"]
    return s, enka, stats.multivariate_normal(mean=prob["mean"], cov=prob["cov"]), prob


def test_refusals_before_any_engine():
    s, enka, prior, prob = _sampler()
    K, p, n = gc.STEP_SHAPE
    mdl = gc.make_model(K, p, n)
    for update in ("langevin", "hmc"):
        with pytest.raises(ValueError, match="fused"):
            s.model_mh(mdl, 4, prior, enka, prob["Gamma"], update=update, chains=4, fused=True)
    noisy = gc.make_model(K, p, n)
    noisy.flag_noise = True
    for update in ("langevin", "hmc"):
        with pytest.raises(ValueError, match="flag_noise"):
            s.model_mh(noisy, 4, prior, enka, prob["Gamma"], update=update, chains=4)
    # the streamed solver keeps no multipliers: a model with the gradient cannot switch to it, one that streams gets no gradient
    with pytest.raises(ValueError, match="streamed"):
        mdl.set_device_solver("streamed")
    streamed = gc.dc.make_model(K, p, n)
    streamed.set_device_solver("streamed")
    with pytest.raises(ValueError, match="streamed"):
        streamed.enable_gradient()
    for update in ("langevin", "hmc"):
        with pytest.raises(ValueError, match="Jacobian"):
            s.model_mh(streamed, 4, prior, enka, prob["Gamma"], update=update, chains=4)
    # a plain model (no enable_gradient) is refused as before, host and device
    plain = gc.dc.make_model(K, p, n)
    for kw in (dict(update="langevin", chains=4), dict(update="hmc", chains=4), dict(update="langevin")):
        with pytest.raises(ValueError, match="Jacobian"):
            s.model_mh(plain, 4, prior, enka, prob["Gamma"], **kw)
    assert not hasattr(s, "samples") and not hasattr(s, "_mh_eng")


def test_the_device_path_accepts_the_gradient_hook():
    """``_model_langevin_refusals`` passes a Darcy model after ``enable_gradient()`` on the device path, and ``model_trunc`` as ``model``."""
    from ces_amd import darcy, sample
    prior = stats.multivariate_normal(mean=np.zeros(10), cov=np.eye(10))
    for mdl in (gc.make_model(*gc.STEP_SHAPE), darcy.model(Nmesh=4.0).enable_gradient()):
        assert hasattr(mdl, "gradient_device") and not hasattr(mdl, "jacobian_device")
        sample.MCMC._model_langevin_refusals(mdl, prior, True)
        sample.MCMC._model_hmc_refusals(mdl, prior, True)
    assert isinstance(gc.make_model(*gc.STEP_SHAPE), darcy.model_trunc)


def test_exact_factors_are_exact():
    """The dense Gamma and prior of the stage cases: L L^{-1} = I with no rounding, the Cholesky factor of L L^T is L, and the
    whitened y is the same bits in a serial sum (the engine's) and in numpy's product."""
    for m, k in ((12, -7), (5, 3), (256, 0), (3, -2)):
        L, Li = cc.exact_factor(m, k)
        assert np.array_equal(L @ Li, np.eye(m)) and np.array_equal(Li @ L, np.eye(m))
        assert np.array_equal(np.linalg.cholesky(L @ L.T), L)
    for K, p, n, M in cc.STAGE_SHAPES:
        sp = cc.stage_problem(K, p, n, M, "dense", "dense", "float64")
        f = sp["f"]
        serial = np.array([sum(f["Lg"][i, k] * sp["y"][k] for k in range(i + 1)) for i in range(n)])
        assert np.array_equal(serial, f["yw"]) and np.array_equal(np.linalg.cholesky(sp["Gamma"]) @ f["Lg"], np.eye(n))
        assert np.array_equal(np.linalg.cholesky(sp["cov"]) @ f["LSi"], np.eye(p))
        assert np.all(np.isfinite(sp["U0"])) and sp["U0"].shape == (p, M) and np.all(np.triu(sp["S"], 1) == 0)


@pytest.mark.parametrize("gkind", ["diag", "dense"])
def test_ready_score_is_the_host_score(gkind):
    """phi and g of the READY formulas from the host adjoint's (G, d) against gc.host_score, and the whole step against
    gc.np_step at L = 1 and 3 on the leading chains: 1e-12 relative."""
    prob = gc.step_problem(gkind)
    f = cc.factors(prob)
    S = cc.step_scale(prob, cc.STEP_DELTA)
    U = np.array(prob["Ustar"][:, :6])
    sc_ = cc.ready_score(f, S, U, *cc.host_grad(prob, U))
    for j in range(U.shape[1]):
        phi, g, _, _ = gc.host_score(prob, S, U[:, j])
        assert abs(sc_["phi"][j] - phi) <= 1e-12 * abs(phi)
        assert np.max(np.abs(sc_["g"][:, j] - g)) <= 1e-12 * np.max(np.abs(g))
        assert sc_["Bphi"][j] >= abs(phi) and np.all(sc_["Bg"][:, j] >= np.abs(g) * (1 - 1e-12))
    for L in (1, 3):
        xi, logu = cc.injected(gkind, L)
        Q, acc, margin, Un = cc.ready_step(prob, f, S, U, xi[:, :6], logu[:6], L)
        Qn, accn, marginn, Unn = gc.np_step(prob, S, U, xi[:, :6], logu[:6], L)
        scale = np.max(np.abs(Qn))
        assert np.max(np.abs(Q - Qn)) <= 1e-12 * scale and np.array_equal(acc, accn)
        assert np.max(np.abs(margin - marginn)) <= 1e-12 * np.max(np.abs(marginn) + 100.0)
        assert np.max(np.abs(Un - Unn)) <= 1e-12 * scale


@pytest.mark.parametrize("L", [1, 3])
@pytest.mark.parametrize("gkind", ["diag", "dense"])
def test_injected_blocks_leave_every_margin_clear(gkind, L):
    """gc.np_step on the blocks the GPU tests inject: |margin| > 1e-6 on every one of the 130 chains, so the device's accept
    decisions are compared on all of them; both outcomes occur."""
    ref = cc.step_reference(gkind, L)
    assert ref["margin"].shape == (gc.M_STEP,) and np.all(np.isfinite(ref["margin"]))
    print("%s L=%d: min |margin| %.3g, accepted %d of %d" % (gkind, L, np.min(np.abs(ref["margin"])), ref["acc"].sum(), gc.M_STEP))
    assert np.min(np.abs(ref["margin"])) > cc.MARGIN_MIN
    assert 10 <= ref["acc"].sum() <= gc.M_STEP - 10
    assert np.all(ref["bound"] > 0) and np.all(np.isfinite(ref["bound"]))
