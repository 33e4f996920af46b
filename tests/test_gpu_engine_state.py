"""The engine's stage state across cesx_set_problem and across its lifetime, through the Python binding alone.

Each stage behind Calibrate keeps a state of its own in the engine (ces_amd/csrc/cesx_stages.h).  A new problem drops the two
that are images of the problem -- the MH proposal and the dense descriptor of mode 'dense' -- and leaves the GP image, the fit
problem and the three forward maps installed; an engine gives all of its device memory back when it is closed, whatever was
installed, re-installed and grown in it."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import darcy_cases as dc  # noqa: E402
import gp_cases as gc  # noqa: E402
import gp_dense_cases as gdc  # noqa: E402
import l96_cases as lc  # noqa: E402

pytestmark = pytest.mark.gpu
MIB = 1 << 20


def _hom_l96(shape, n_t=21):
    """The homogeneous Lorenz '96 model (statistics averaged over the slow index: p = 4, n_obs = 5) at ``shape``."""
    m = lc.make_model("lorenz96_hom", T=0.2)
    m.n_slow, m.n_fast = shape
    m.n_state = shape[0] * (shape[1] + 1)
    return m, lc.times(0.2, n=n_t)


def _fit_theta(n, p):
    """(sigma^2, p lengthscales, sn^2) per GP: ARD, zero mean."""
    return np.hstack([np.full((n, 1), 1.3), np.tile(1.0 + 0.25 * np.arange(p), (n, 1)), np.full((n, 1), 1e-3)])


def test_set_problem_drops_what_it_should_and_nothing_else():
    """One fp64 engine of the smallest shape every stage admits (p = 4, n_obs = 5: Darcy K = 4, the homogeneous Lorenz '96
    model at (5, 3)), J = 65.  Every stage installed and called once; then a second problem.  The proposal and the dense
    descriptor are gone (the state errors of cesx_mh_propose / cesx_mh_accept / cesx_gp_start), and gp_predict, gpfit_eval,
    darcy_apply, l96_apply and forward_apply return what they returned before, bit for bit: the same kernels on the same
    tables, no tolerance."""
    import torch
    from ces_amd import emulate as em
    from ces_amd import engine
    p, n, J, k = 4, 5, 65, 3
    rng = np.random.default_rng(20260)
    eng = engine.Engine(p, n, J, dtype="float64")
    pr = gdc.problem(rng, n, k, 10.0, "pca", p=p, dense_prior=True)          # dense Gamma, dense Sigma
    pr2 = gdc.problem(rng, n, k, 100.0, "pca", p=p, dense_prior=True)
    eng.set_problem(pr["y"], pr["Gamma"], pr["mu"], pr["Sp"], pr["mu"])

    # the three forward maps
    U = eng.to_device(gdc.states(rng, pr, J), p, "U")
    A, b = rng.standard_normal((n, p)), rng.standard_normal(n)
    eng.forward_set_lineal(A, b)
    darcy = dc.make_model(4, p, n)
    Ud = eng.to_device(rng.standard_normal((p, J)), p, "Ud")
    params, starts = lc.class_params("lorenz96", (5, 3))
    l96, t = _hom_l96((5, 3))
    Ul = eng.to_device(np.array(params[:, :J]), p, "Ul")
    Wl = torch.as_tensor(np.array(starts[:, :J]), device=eng.device)
    # the GP image (J_t = 17, 3 GPs) and the fit problem (J_t = 17)
    enka = gc.random_gps(rng, p, k, 17, "Matern32")
    eng.gp_set(em.device_image(enka, enka.gpmodels))
    Xf, Yf = gc.fit_problem(rng, 17, p, 2)
    nt = eng.gpfit_set(Xf, Yf, 2, True, "zero")
    theta = _fit_theta(2, p)
    assert theta.shape == (2, nt)

    def outputs():
        l96.ensure_installed(eng, t)
        Gl, W_out, info = eng.l96_apply(Ul, Wl)
        m, v = eng.gp_predict(U)
        out = dict(fwd=eng.forward_apply(U), darcy=darcy.forward_device(eng, Ud), l96_G=Gl, l96_W=W_out, l96_info=info,
                   gp_mean=m, gp_var=v)
        out = {key: val.cpu().numpy().copy() for key, val in out.items()}
        lml, grad, status = eng.gpfit_eval([1, 0], theta)
        out.update(fit_lml=lml, fit_grad=grad, fit_status=status)
        assert np.all(out["l96_info"][0] == 0) and np.all(status == engine.OK)
        return out

    before = outputs()
    assert all(np.all(np.isfinite(v)) for v in before.values())
    # the two chain starts: phi from the model's G, and from the GP rows in mode 'dense'
    S = 0.3 * np.linalg.cholesky(pr["Sp"])
    eng.mh_set_proposal(None, S)
    eng.gp_dense_set(pr["B"], pr["g0"], True)
    G = eng.forward_apply(U)
    eng.mh_start(U, G)
    phi_mh = eng.mh_phi()
    md, vd = eng.gp_predict(U)
    eng.gp_start("dense", U, md, vd)
    phi_gp = eng.mh_phi()
    assert np.all(np.isfinite(phi_mh)) and np.all(np.isfinite(phi_gp)) and not np.array_equal(phi_mh, phi_gp)
    P = eng.mh_propose(0, U)
    eng.mh_accept(0, U.clone(), P, eng.forward_apply(P))

    eng.set_problem(pr2["y"], pr2["Gamma"], pr2["mu"], pr2["Sp"], pr2["mu"])

    # dropped: the proposal (and the chains started under it) ...
    for call, word in ((lambda: eng.mh_propose(1, U), "cesx_mh_set_proposal has not been called"),
                       (lambda: eng.mh_accept(1, U.clone(), P, G), "cesx_mh_start has not been called"),
                       (lambda: eng.gp_start("dense", U, md, vd), "no proposal"),
                       (lambda: eng.mh_phi(), "no start")):
        with pytest.raises(engine.CesxError) as ei:
            call()
        assert ei.value.code == engine.ESTATE and word in str(ei.value), str(ei.value)
    # ... and the dense descriptor: with a proposal again, mode 'dense' still has nothing to score with
    eng.mh_set_proposal(None, 0.3 * np.linalg.cholesky(pr2["Sp"]))
    with pytest.raises(engine.CesxError) as ei:
        eng.gp_start("dense", U, md, vd)
    assert ei.value.code == engine.ESTATE and "cesx_gp_dense_set" in str(ei.value)
    # kept: everything else, bit for bit
    after = outputs()
    assert sorted(after) == sorted(before)
    for key in before:
        assert np.array_equal(before[key], after[key]), key
    eng.close()


def _free_bytes():
    import torch
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    return torch.cuda.mem_get_info()[0]


CYCLES = 8
SLACK = 1 * MIB


def test_create_reinstall_destroy_returns_device_memory():
    """8 cycles (after one warm-up cycle) of: create (p = 4, n_obs = 5, J = 65536, fp64: every J-sized buffer is 2 MiB or
    more), set_problem with a dense Gamma and a dense Sigma, the GP image at J_t = 1024 and then 700 (2 GPs: 4.2 / 2.0 MiB
    of L^{-1} each), a gp_predict behind each (past the LDS limit: the K* workspace, 256 MiB, is grown once and kept), the
    fit problem at J_t = 512 and then 300 (2 GPs), the Darcy map at K = 8 and then 4 and the Lorenz '96 map with 41 and then
    21 sample times (installed only: their tables are a few KiB, which this test cannot see -- tools/devbuf_check.cpp
    covers them), the MH proposal with the dense prior's images and the fp64 noise block, the dense descriptor, one
    prefetch_noise, close().

    Free device memory after cycle 8 must not lie below free memory after cycle 1 by more than SLACK.  One buffer of 2 MiB
    leaked per cycle would cost 14 MiB over the 7 cycles between the two readings.  SLACK is twice the largest |free_8 -
    free_1| of three runs of this loop at the commit before the stage structs, with a floor of 1 MiB; it has to stay below
    8 MiB.  Those three drifts: 0, 0, 0 bytes -> SLACK = 1 MiB (NOTEBOOK.md, "Who owns device memory")."""
    import torch
    from ces_amd import emulate as em
    from ces_amd import engine
    p, n, J, k = 4, 5, 65536, 2
    rng = np.random.default_rng(20261)
    pr = gdc.problem(rng, n, k, 10.0, "pca", p=p, dense_prior=True)
    images = []
    for Jt in (1024, 700):
        enka = gc.random_gps(rng, p, k, Jt, "Matern32")
        images.append(em.device_image(enka, enka.gpmodels))
    fits = [gc.fit_problem(rng, Jt, p, 2) for Jt in (512, 300)]
    darcys = [dc.make_model(K, p, n) for K in (8, 4)]
    l96s = [_hom_l96((5, 3), n_t) for n_t in (41, 21)]
    X = (pr["mu"][:, None] + 0.5 * rng.standard_normal((p, J)))
    S = 0.3 * np.linalg.cholesky(pr["Sp"])

    def cycle():
        eng = engine.Engine(p, n, J, dtype="float64")
        eng.set_problem(pr["y"], pr["Gamma"], pr["mu"], pr["Sp"], pr["mu"])
        Xd = eng.to_device(X, p, "X")
        for img in images:
            eng.gp_set(img)
            m, v = eng.gp_predict(Xd)
        assert bool(torch.isfinite(m).all()) and bool(torch.isfinite(v).all())
        for Xf, Yf in fits:
            eng.gpfit_set(Xf, Yf, 2, True, "zero")
        for mdl in darcys:
            mdl.invalidate_device()
            mdl.ensure_installed(eng)
        for mdl, t in l96s:
            mdl.invalidate_device()
            mdl.ensure_installed(eng, t)
        eng.mh_set_proposal(None, S)
        eng.gp_dense_set(pr["B"], pr["g0"], True)
        eng.prefetch_noise(0)
        eng.close()
        del eng, Xd, m, v
        return _free_bytes()

    cycle()                                        # warm-up: the runtime's own pools, the kernels' code objects
    free = [cycle() for _ in range(CYCLES)]
    drift = free[-1] - free[0]
    print("\n[engine state] free device memory after cycles 1..%d, MiB below the first: %s; free_8 - free_1 = %d bytes"
          % (CYCLES, ["%.2f" % ((free[0] - f) / MIB) for f in free], drift))
    assert SLACK < 8 * MIB
    assert free[-1] >= free[0] - SLACK, (drift, free)
