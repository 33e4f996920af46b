"""The gradient samplers on the projected Sigma, on the device (kernels_gpprojgrad.hip; cesx_gp_proj_coef, cesx_gp_proj_langevin_*
and cesx_gp_proj_hmc_*; gp_mh(chains=, pca_tools=, sigma_form='projected', update='langevin' / 'hmc')).

The coefficients are held ELEMENTWISE through gp_proj_coef on crafted rows (not through the GP) against the literal n-space
form within the bars of tests/gp_proj_grad_cases.py (the measurement behind their constants is in that module); g through a
proposal with xi = 0; the accept step against a reference chain with the band max(1e-9 max(1, |phi|), bound(U) + bound(P) + the
correction's propagated bound) and the cap of 1 chain-step in 1000 left out; guards around every buffer a kernel may write.

Worst ratios to the bars are printed (pytest -s) and recorded in NOTEBOOK.md."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gp_dense_cases as gc  # noqa: E402
import gp_proj_cases as gq  # noqa: E402
import gp_proj_grad_cases as gg  # noqa: E402
from edge_helpers import guarded, guards_intact, put, same_bits  # noqa: E402
from test_emulate_host import gold_prior, load_gold  # noqa: E402
from test_gpu_gp_dense import dev, trivial_image  # noqa: E402
from test_gpu_gp_proj import stretched  # noqa: E402
from test_gpu_sample_edges import eng_mod, note  # noqa: E402,F401

from oracle import stage_ref as sr  # noqa: E402

pytestmark = pytest.mark.gpu
EPS = gg.EPS
SCALE = 0.3                # the proposal's S = SCALE chol(Sigma_prior)


def engine(eng_mod, pr, M, dtype, kind, logdet, **kw):
    eng = eng_mod.Engine(pr["p"], pr["n"], M, dtype=dtype, **kw)
    eng.set_problem(pr["y"], pr["Gamma"], pr["mu"], pr["Sp"], pr["mu"])
    S = SCALE * np.linalg.cholesky(pr["Sp"])
    eng.mh_set_proposal(kind, S, 0.5)
    eng.gp_set(trivial_image(pr["p"], pr["k"]))
    eng.gp_proj_set(*gq.project(pr), logdet)
    return eng, S


def guarded64(eng, rows):
    """``guarded`` in float64 whatever the engine dtype: the coefficient launch writes fp64."""
    import torch
    from edge_helpers import GUARD, SENTINEL
    flat = torch.full((2 * GUARD + rows * eng.J,), SENTINEL, dtype=torch.float64, device=eng.device)
    return flat, flat[GUARD:GUARD + rows * eng.J].view(rows, eng.J)


def coef(eng, m, v, bufs=None):
    """gp_proj_coef on the rows -> (phi_data, a, b) on the host; the rows untouched."""
    md, vd = dev(eng, np.array(m)), dev(eng, np.array(v))      # (copies: coef_case's arrays are read-only)
    out = None if bufs is None else (bufs[0][1][0], bufs[1][1], bufs[2][1])
    ph, a, b = eng.gp_proj_coef(md, vd, out=out)
    res = ph.cpu().numpy(), a.cpu().numpy(), b.cpu().numpy()
    assert np.array_equal(md.cpu().numpy(), m) and np.array_equal(vd.cpu().numpy(), v, equal_nan=True)
    return res


# ---- the coefficients, elementwise -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("M", gq.GPU_M)
@pytest.mark.parametrize("n,k", gq.GPU_SHAPES)
def test_coefficients_elementwise(eng_mod, n, k, M):
    """(one problem of 257 chains per shape, its literal reference computed once; M chains of it per case, both log det values)"""
    assert gq.GPU_M == [1, 5, 257]
    pr, m_all, v_all, ref = gg.coef_case(n, k, 257)
    cols = slice(0, M) if M > 1 else slice(200, 201)
    m, v = np.ascontiguousarray(m_all[:, cols]), np.ascontiguousarray(v_all[:, cols])
    for logdet in (False, True):
        eng, _ = engine(eng_mod, pr, M, "float64", "langevin", logdet)
        bufs = [guarded64(eng, 1), guarded64(eng, k), guarded64(eng, k)]
        ph, a, b = coef(eng, m, v, bufs)
        r = gg.take(ref, logdet, cols)
        bar_phi, bar_e, _, bar_b = gg.bars(pr, r, logdet)
        rp, ra, rb = (float(np.max(x)) for x in (np.abs(ph - r["phi"]) / bar_phi, np.abs(a - r["e"]) / bar_e,
                                                 np.abs(b - gg.coef_b(r["e"], r["h"], logdet)) / bar_b))
        w = [note("projgrad %s" % key, ratio=val)["ratio"] for key, val in (("phi_data", rp), ("a", ra), ("b", rb))]
        print("gp_proj_coef n=%d k=%d M=%d logdet=%d: cond up to %.1e, worst ratios to the bars phi_data %.3g a %.3g b %.3g "
              "(so far %.3g %.3g %.3g)" % (n, k, M, logdet, r["cond"].max(), rp, ra, rb, *w))
        assert rp <= 1.0 and ra <= 1.0 and rb <= 1.0, (logdet, rp, ra, rb)
        assert all(guards_intact(f, view) for f, view in bufs)


# ---- determinism -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [3, 16, 33, 128])
def test_bits_do_not_depend_on_the_call_the_column_the_group_or_the_neighbours(eng_mod, k):
    n, M = 129, 257
    pr, m, v, _ = gg.coef_case(n, k, M)
    eng, _ = engine(eng_mod, pr, M, "float64", "langevin", True)
    one, two = coef(eng, m, v), coef(eng, m, v)
    assert all(np.all(np.isfinite(x)) and np.all(same_bits(x, y)) for x, y in zip(one, two))
    eng1, _ = engine(eng_mod, pr, 1, "float64", "langevin", True)
    for col in (0, 1, 2, 3, 64, 255, 256):                   # every group of a wave, a later wave, the ragged last wave
        alone = coef(eng1, np.ascontiguousarray(m[:, [col]]), np.ascontiguousarray(v[:, [col]]))
        assert all(np.all(same_bits(x[..., 0], y[..., col])) for x, y in zip(alone, one)), col
    rng = np.random.default_rng([k, 5])                      # other neighbours, same bits
    m2, v2 = gc.rows(rng, k, M)
    m2[:, 65], v2[:, 65] = m[:, 2], v[:, 2]
    three = coef(eng, m2, v2)
    assert all(np.all(same_bits(x[..., 65], y[..., 2])) for x, y in zip(three, one))


# ---- crafted gradients: what lv_score makes of the coefficients -----------------------------------------------------------

def crafted_grads(rng, k, p, M, lit=None, logdet=True):
    """Crafted gradients of the GP rows (k, p, M).  With ``lit`` (``gg.literal``'s dict of the rows they go with) row t of chain j
    is scaled by 1 / (sqrt(k) |a_tj|) resp. 1 / (sqrt(k) |b_tj|), so that the data term of grad phi is of order one per
    component whatever the coefficients' size, and an accept loop both takes and refuses."""
    dm, dv = rng.standard_normal((k, p, M)), rng.standard_normal((k, p, M))
    if lit is None:
        return 0.5 * dm, 0.1 * dv
    with np.errstate(invalid="ignore", divide="ignore"):
        sm = 1.0 / (np.sqrt(k) * np.abs(lit["e"]))
        sv = 1.0 / (np.sqrt(k) * np.abs(gg.coef_b(lit["e"], lit["h"], logdet)))
    sm, sv = (np.where(np.isfinite(x), x, 1.0) for x in (sm, sv))
    return dm * sm[:, None, :], dv * sv[:, None, :]


def literal_phi_g(pr, S, ref, logdet, X, dm, dv):
    """(phi, its bar, g = S^T grad phi, its bar (p, M)) from ``literal``'s dict at the states X (p, M): the coefficients' bars
    carried through |grad m| and |grad v|, plus (p + 8) eps of the prior term's absolute values, then through |S^T|."""
    p = pr["p"]
    bar_phi, bar_e, _, bar_b = gg.bars(pr, ref, logdet)
    pt, pt_abs = gc.prior_term(pr, X)
    b = gg.coef_b(ref["e"], ref["h"], logdet)
    du = np.asarray(X, dtype=np.float64) - pr["mu"][:, None]
    Si = np.linalg.inv(pr["Sp"])
    grad = np.einsum("tj,tqj->qj", ref["e"], dm) + np.einsum("tj,tqj->qj", b, dv) + Si @ du
    bar = np.einsum("tj,tqj->qj", bar_e, np.abs(dm)) + np.einsum("tj,tqj->qj", bar_b, np.abs(dv)) + (p + 8) * EPS * (np.abs(Si) @ np.abs(du))
    return ref["phi"] + pt, bar_phi + (p + 8) * EPS * pt_abs, S.T @ grad, np.abs(S.T) @ bar


@pytest.mark.parametrize("dense_prior", [False, True])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_the_start_leaves_gp_starts_phi_bit_for_bit(eng_mod, dtype, dense_prior):
    """phi of gp_langevin_start('proj') is phi of gp_start('proj') on the same rows and states (k = 4, 16, 33, 128)."""
    for n, k in ((129, 4), (180, 16), (129, 33), (180, 128)):
        M = 70
        rng = np.random.default_rng([n, k, int(dense_prior), 3])
        pr = gc.problem(rng, n, k, 1e4, "pca", dense_prior=dense_prior)
        m, v = gc.rows(rng, k, M)
        dm, dv = crafted_grads(rng, k, pr["p"], M)
        Uh = gc.states(rng, pr, M, np.dtype(dtype))
        for logdet in (False, True):
            phis = []
            for kind in (None, "langevin"):
                eng, _ = engine(eng_mod, pr, M, dtype, kind, logdet)
                U_flat, U = guarded(eng, pr["p"])
                put(U, Uh)
                if kind is None:
                    eng.gp_start("proj", U, dev(eng, m), dev(eng, v))
                else:
                    eng.gp_langevin_start("proj", U, dev(eng, m), dev(eng, v), dev(eng, dm), dev(eng, dv))
                phis.append(eng.mh_phi())
                assert guards_intact(U_flat, U) and np.all(same_bits(U.cpu().numpy(), Uh))
            assert np.all(np.isfinite(phis[0])) and np.array_equal(phis[0], phis[1]), (n, k, logdet)


@pytest.mark.parametrize("n,k", [(129, 4), (180, 16), (129, 33), (180, 128)])
def test_g_through_a_proposal_without_noise(eng_mod, n, k):
    """gp_langevin_propose with xi = 0 in the fp64 engine: P - U = -1/2 S g.  The bar: |S| bar(g) / 2, bar(g) as literal_phi_g
    carries it, plus the store of P = U + (...), which rounds once: eps (|U| + |P - U|)."""
    M = 70
    for logdet, dense_prior in ((True, False), (False, True)):
        rng = np.random.default_rng([n, k, int(logdet), 8])
        pr = gc.problem(rng, n, k, 1e4, "pca", dense_prior=dense_prior)
        p = pr["p"]
        m, v = gc.rows(rng, k, M)
        dm, dv = crafted_grads(rng, k, p, M)
        Uh = gc.states(rng, pr, M)
        ref = gg.literal(pr, m, v, logdet)
        assert np.all(ref["cond_s"] <= gc.COND_SCORE)
        eng, S = engine(eng_mod, pr, M, "float64", "langevin", logdet)
        U_flat, U = guarded(eng, p)
        P_flat, P = guarded(eng, p)
        put(U, Uh)
        eng.gp_langevin_start("proj", U, dev(eng, m), dev(eng, v), dev(eng, dm), dev(eng, dv))
        eng.gp_langevin_propose(0, U, xi=dev(eng, np.zeros((p, M))), out=P)
        step = P.cpu().numpy() - Uh
        _, _, g, bar_g = literal_phi_g(pr, S, ref, logdet, Uh, dm, dv)
        want = -0.5 * (S @ g)
        bar = 0.5 * (np.abs(S) @ bar_g) + EPS * (np.abs(Uh) + np.abs(want))
        ratio = float(np.max(np.abs(step - want) / bar))
        print("g n=%d k=%d logdet=%d: worst |P - U + S g / 2| / bar %.3g (so far %.3g)"
              % (n, k, logdet, ratio, note("projgrad g", ratio=ratio)["ratio"]))
        assert ratio <= 1.0 and np.all(np.abs(want) > 0)
        assert guards_intact(U_flat, U) and guards_intact(P_flat, P)


# ---- the accept step -----------------------------------------------------------------------------------------------------------

ACCEPT_STEPS = 6


def accept_reference(n, k, M, dtype, seed):
    """The problem and the generator of one accept case: every step draws its noise block, its uniforms, its crafted rows and
    their gradients from the generator in one order, with or without a device."""
    ndt = np.dtype(dtype)
    rng = np.random.default_rng([n, k, M, ndt.itemsize, seed])
    pr = gc.problem(rng, n, k, 1e2, "pca", dense_prior=(seed % 2 == 1), b_scale=(-2.0, 0.0))
    return pr, rng, ndt


def run_accept(eng_mod, n, k, M, dtype, seed, device=True):
    """ACCEPT_STEPS Langevin steps of M chains on crafted rows and gradients: the device proposes from its own g (held to the
    literal g's bar) and accepts; the literal reference scores the same proposal and decides; outside the band the decisions
    agree, inside it the reference follows the device.  device=False: the kernel-order restatement stands in for the device
    (the CPU check of the cap, tests/test_gp_proj_grad_host.py)."""
    logdet = True
    pr, rng, ndt = accept_reference(n, k, M, dtype, seed)
    p = pr["p"]
    S = SCALE * np.linalg.cholesky(pr["Sp"])
    proj = gq.project(pr)

    def rows_and_grads():
        m, v = gc.rows(rng, k, M, v_lo=1e-6)
        r = gg.literal(pr, m, v, logdet)
        assert np.all(r["cond_s"] <= gc.COND_ACCEPT)
        return (m, v) + crafted_grads(rng, k, p, M, r, logdet) + (r,)

    def ref_of(Xh, r, dm, dv):
        return literal_phi_g(pr, S, r, logdet, Xh.astype(np.float64), dm, dv)

    def restated(Xh, m, v, dm, dv):
        ph, a, b = gg.kernel_order_proj_coef(pr, m, v, logdet, proj=proj)
        du = Xh.astype(np.float64) - pr["mu"][:, None]
        grad = np.einsum("tj,tqj->qj", a, dm) + np.einsum("tj,tqj->qj", b, dv) + np.linalg.solve(pr["Sp"], du)
        return ph + gc.prior_term(pr, Xh)[0], S.T @ grad

    Uh = gc.states(rng, pr, M, ndt)
    m, v, dm, dv, lit = rows_and_grads()
    phi_u, bar_u, g_u, bg_u = ref_of(Uh, lit, dm, dv)
    if device:
        eng, _ = engine(eng_mod, pr, M, dtype, "langevin", logdet)
        U_flat, U = guarded(eng, p)
        P_flat, P = guarded(eng, p)
        put(U, Uh)
        eng.gp_langevin_start("proj", U, dev(eng, m), dev(eng, v), dev(eng, dm), dev(eng, dv))
        assert np.all(np.abs(eng.mh_phi() - phi_u) <= bar_u)
    else:
        phi_k, g_k = restated(Uh, m, v, dm, dv)
    left_out = taken_total = 0
    for step in range(ACCEPT_STEPS):
        xi = rng.standard_normal((p, M)).astype(ndt)
        logu = np.log(rng.random(M))
        m, v, dm, dv, lit = rows_and_grads()
        if device:                                           # the device's own proposal, from its own g
            eng.gp_langevin_propose(step, U, xi=dev(eng, xi).to(eng.torch_dtype), out=P)
            Ph = P.cpu().numpy()
            want = Uh.astype(np.float64) + S @ (xi.astype(np.float64) - 0.5 * g_u)
            tol = 0.5 * (np.abs(S) @ bg_u) + (EPS if dtype == "float64" else 2.0 ** -23) * (np.abs(Uh) + np.abs(want))
            assert np.all(np.abs(Ph - want) <= tol), float(np.max(np.abs(Ph - want) / tol))
        else:
            Ph = (Uh.astype(np.float64) + S @ (xi.astype(np.float64) - 0.5 * g_k)).astype(ndt)
        phi_p, bar_p, g_p, bg_p = ref_of(Ph, lit, dm, dv)
        back = xi.astype(np.float64) - 0.5 * (g_u + g_p)
        corr = 0.5 * (xi.astype(np.float64) ** 2).sum(axis=0) - 0.5 * (back * back).sum(axis=0)
        hb = 0.5 * (bg_u + bg_p)                             # the bar of (g_U + g_P) / 2, carried through |back|^2 / 2
        bar_corr = (np.abs(back) * hb).sum(axis=0) + 0.5 * (hb * hb).sum(axis=0)
        margin = phi_u - phi_p + corr - logu
        band = np.abs(margin) <= np.maximum(sr.BAND * np.maximum(1.0, np.abs(phi_u)), bar_u + bar_p + bar_corr)
        accept = margin > 0
        if device:
            eng.gp_langevin_accept("proj", step, U, P, dev(eng, m), dev(eng, v), dev(eng, dm), dev(eng, dv), logu=dev(eng, logu))
            Un = U.cpu().numpy()
            took, kept = np.all(same_bits(Un, Ph), axis=0), np.all(same_bits(Un, Uh), axis=0)
            assert np.all(took | kept) and guards_intact(U_flat, U) and guards_intact(P_flat, P)
        else:
            phi_pk, g_pk = restated(Ph, m, v, dm, dv)
            bk = xi.astype(np.float64) - 0.5 * (g_k + g_pk)
            took = logu < phi_k - phi_pk + (0.5 * (xi.astype(np.float64) ** 2).sum(axis=0) - 0.5 * (bk * bk).sum(axis=0))
            phi_k, g_k = np.where(took, phi_pk, phi_k), np.where(took, g_pk, g_k)
        assert np.all((took == accept) | band), (step, np.flatnonzero((took != accept) & ~band)[:8])
        left_out += int(band.sum())
        taken_total += int(took.sum())
        Uh = np.where(took, Ph, Uh)                          # the reference follows the decisions that hold (the device's in the band)
        phi_u, bar_u = np.where(took, phi_p, phi_u), np.where(took, bar_p, bar_u)
        g_u, bg_u = np.where(took, g_p, g_u), np.where(took, bg_p, bg_u)
    if device:
        assert np.all(np.abs(eng.mh_phi() - phi_u) <= bar_u)
        nsteps, rate, per = eng.mh_stats(per_chain=True)
        assert nsteps == ACCEPT_STEPS and per.sum() == taken_total
    w = note("projgrad accept" if device else "projgrad accept (restatement)")
    w["left_out"] += left_out
    w["chain_steps"] += ACCEPT_STEPS * M
    print("langevin accept proj %s n=%d k=%d M=%d %s: %d of %d chain-steps taken, %d inside the band"
          % (dtype, n, k, M, "device" if device else "restatement", taken_total, ACCEPT_STEPS * M, left_out))
    assert 0 < taken_total < ACCEPT_STEPS * M
    assert 1000 * left_out <= ACCEPT_STEPS * M, left_out


ACCEPT_CASES = [(129, 4, "float64", 0), (129, 4, "float32", 1), (180, 128, "float64", 2), (180, 128, "float32", 3)]


@pytest.mark.parametrize("n,k,dtype,seed", ACCEPT_CASES)
def test_accept_step(eng_mod, n, k, dtype, seed):
    run_accept(eng_mod, n, k, 257, dtype, seed)


# ---- leapfrog = 1 -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [4, 33])
def test_one_leapfrog_is_the_langevin_step_bit_for_bit(eng_mod, k):
    n, M, steps = 129, 33, 8
    rng = np.random.default_rng([n, k, 17])
    pr = gc.problem(rng, n, k, 1e2, "pca", b_scale=(-2.0, 0.0))
    p = pr["p"]
    Uh = gc.states(rng, pr, M)
    data = []
    for _ in range(steps + 1):
        m, v = gc.rows(rng, k, M, v_lo=1e-6)
        data.append(((m, v), crafted_grads(rng, k, p, M, gg.literal(pr, m, v, True)), rng.standard_normal((p, M)), np.log(rng.random(M))))
    out = []
    for hmc in (False, True):
        eng, _ = engine(eng_mod, pr, M, "float64", "langevin", True)
        _, U = guarded(eng, p)
        _, P = guarded(eng, p)
        put(U, Uh)
        (m, v), (dm, dv), _, _ = data[0]
        eng.gp_langevin_start("proj", U, dev(eng, m), dev(eng, v), dev(eng, dm), dev(eng, dv))
        trace = []
        for step in range(steps):
            (m, v), (dm, dv), xi, logu = data[step + 1]
            rows = dev(eng, m), dev(eng, v), dev(eng, dm), dev(eng, dv)
            if hmc:
                eng.mh_hmc_begin(step, U, xi=dev(eng, xi), out=P)
                eng.gp_hmc_accept("proj", step, U, P, *rows, logu=dev(eng, logu))
            else:
                eng.gp_langevin_propose(step, U, xi=dev(eng, xi), out=P)
                eng.gp_langevin_accept("proj", step, U, P, *rows, logu=dev(eng, logu))
            trace.append((U.cpu().numpy().copy(), eng.mh_phi()))
        out.append(trace)
        _, rate, _ = eng.mh_stats(per_chain=True)
        assert 0.0 < rate < 1.0
    for (u1, p1), (u2, p2) in zip(*out):
        assert np.all(same_bits(u1, u2)) and np.all(same_bits(p1, p2))


# ---- an indefinite Sigma ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [4, 16, 33])
def test_an_indefinite_sigma_is_nan_rejects_and_leaves_its_wave_alone(eng_mod, k):
    """v = -10 in one chain of 257 (k = 4: chains 36 .. 39 share its wave; k = 16: 148 .. 151; k = 33: alone)."""
    n, M = 129, 257
    bad = {4: 37, 16: 150, 33: 64}[k]
    rng = np.random.default_rng([n, k, 13])
    pr = gc.problem(rng, n, k, 1e2, "pca", b_scale=(-2.0, 0.0))
    p = pr["p"]
    eng, S = engine(eng_mod, pr, M, "float64", "langevin", True)
    m, v = gc.rows(rng, k, M, v_lo=1e-6)
    dm, dv = crafted_grads(rng, k, p, M, gg.literal(pr, m, v, True))
    clean = coef(eng, m, v)
    vb = v.copy()
    vb[1 % k, bad] = -10.0
    assert np.linalg.eigvalsh(gc.sigma_of(pr, vb[:, bad])).min() < 0.0
    got = coef(eng, m, vb)
    good = np.arange(M) != bad
    for x, y in zip(got, clean):
        assert np.all(np.isnan(x[..., bad])) and np.all(same_bits(x[..., good], y[..., good]))
    # a start state in it stays stuck: a proposal any finite phi would take is refused
    U_flat, U = guarded(eng, p)
    P_flat, P = guarded(eng, p)
    Uh = gc.states(rng, pr, M)
    put(U, Uh)
    eng.gp_langevin_start("proj", U, dev(eng, m), dev(eng, vb), dev(eng, dm), dev(eng, dv))
    assert np.isnan(eng.mh_phi()[bad]) and np.all(np.isfinite(eng.mh_phi()[good]))
    m2, v2 = gc.rows(rng, k, M, v_lo=1e-6)
    dm2, dv2 = crafted_grads(rng, k, p, M, gg.literal(pr, m2, v2, True))
    lu = dev(eng, np.full(M, -1e6))
    eng.gp_langevin_propose(0, U, xi=dev(eng, 0.1 * rng.standard_normal((p, M))), out=P)
    Ph = P.cpu().numpy()
    eng.gp_langevin_accept("proj", 0, U, P, dev(eng, m2), dev(eng, v2), dev(eng, dm2), dev(eng, dv2), logu=lu)
    Un = U.cpu().numpy()
    assert np.all(same_bits(Un[:, bad], Uh[:, bad])) and np.all(same_bits(Un[:, good], Ph[:, good]))
    _, _, per = eng.mh_stats(per_chain=True)
    assert per[bad] == 0 and np.all(per[good] == 1) and np.isnan(eng.mh_phi()[bad])
    # ... and a proposal into it is rejected by a chain with a finite phi
    put(U, Uh)
    eng.gp_langevin_start("proj", U, dev(eng, m), dev(eng, v), dev(eng, dm), dev(eng, dv))
    before = eng.mh_phi()
    eng.gp_langevin_propose(0, U, xi=dev(eng, 0.1 * rng.standard_normal((p, M))), out=P)
    Ph = P.cpu().numpy()
    v2b = v2.copy()
    v2b[0, bad] = -10.0
    eng.gp_langevin_accept("proj", 0, U, P, dev(eng, m2), dev(eng, v2b), dev(eng, dm2), dev(eng, dv2), logu=lu)
    Un = U.cpu().numpy()
    assert np.all(same_bits(Un[:, bad], Uh[:, bad])) and np.all(same_bits(Un[:, good], Ph[:, good]))
    after = eng.mh_phi()
    assert same_bits(after[[bad]], before[[bad]])[0] and np.all(np.isfinite(after))
    assert guards_intact(U_flat, U) and guards_intact(P_flat, P)


# ---- ABI states -----------------------------------------------------------------------------------------------------------------

def test_abi_states(eng_mod):
    rng = np.random.default_rng(4)
    n, k, M = 7, 3, 5
    pr = gc.problem(rng, n, k, 1e2, "pca")
    p = pr["p"]
    eng = eng_mod.Engine(p, n, M, dtype="float64")
    eng.set_problem(pr["y"], pr["Gamma"], pr["mu"], pr["Sp"], pr["mu"])
    S = SCALE * np.linalg.cholesky(pr["Sp"])
    eng.mh_set_proposal("langevin", S)
    eng.gp_set(trivial_image(p, k))
    _, U = guarded(eng, p)
    _, P = guarded(eng, p)
    Uh = gc.states(rng, pr, M)
    put(U, Uh)
    m, v = gc.rows(rng, k, M)
    dm, dv = crafted_grads(rng, k, p, M)
    rows = dev(eng, m), dev(eng, v), dev(eng, dm), dev(eng, dv)

    def refused(code, text, call, *args, **kw):
        with pytest.raises((eng_mod.CesxError, ValueError)) as ei:
            call(*args, **kw)
        assert getattr(ei.value, "code", eng_mod.EINVAL) == code and text in str(ei.value), (code, str(ei.value))
    refused(eng_mod.ESTATE, "cesx_gp_proj_set", eng.gp_proj_coef, rows[0], rows[1])                   # no descriptor
    refused(eng_mod.ESTATE, "cesx_gp_proj_set", eng.gp_langevin_start, "proj", U, *rows)
    eng.gp_proj_set(*gq.project(pr), True)
    refused(eng_mod.ESTATE, "cesx_gp_langevin_start", eng.gp_langevin_accept, "proj", 0, U, P, *rows)  # sequencing: no start
    refused(eng_mod.ESTATE, "start", eng.gp_hmc_accept, "proj", 0, U, P, *rows)
    eng.gp_set(trivial_image(p, n))                                                                   # n_gp != k
    refused(eng_mod.EINVAL, "n_gp", eng.gp_langevin_start, "proj", U, *rows)
    img = trivial_image(p, k)
    img["family"] = np.array([0, 1, 0], dtype=np.int32)                                               # a Matern12 image
    eng.gp_set(img)
    refused(eng_mod.EUNSUPPORTED, "Matern12", eng.gp_langevin_start, "proj", U, *rows)
    refused(eng_mod.EUNSUPPORTED, "Matern12", eng.gp_proj_coef, rows[0], rows[1])
    eng.gp_set(trivial_image(p, k))
    refused(eng_mod.EINVAL, "null", eng.gp_langevin_start, "proj", U, rows[0], None, rows[2], None)   # null var / dvar
    refused(eng_mod.EINVAL, "null", eng.gp_langevin_start, "proj", U, rows[0], rows[1], rows[2], None)
    for mode in ("dense", "proj"):                                                                    # the old calls: modes 3 and 4
        rc = eng.lib.cesx_gp_langevin_start(eng._h, eng_mod.GP_MODES[mode], U.data_ptr(), *(r.data_ptr() for r in rows), None)
        assert rc == eng_mod.EINVAL
    eng.gp_langevin_start("proj", U, *rows)
    phi0 = eng.mh_phi()
    refused(eng_mod.ESTATE, "propose", eng.gp_langevin_accept, "proj", 0, U, P, *rows)                # no propose yet
    refused(eng_mod.ESTATE, "cesx_mh_hmc_begin", eng.gp_hmc_leap, "proj", P, *rows)                   # no begin yet
    refused(eng_mod.ESTATE, "cesx_mh_hmc_begin", eng.gp_hmc_accept, "proj", 0, U, P, *rows)
    for mode in ("dense", "proj"):
        rc = eng.lib.cesx_gp_hmc_leap(eng._h, eng_mod.GP_MODES[mode], P.data_ptr(), *(r.data_ptr() for r in rows), None)
        assert rc in (eng_mod.EINVAL, eng_mod.ESTATE)
    eng.mh_hmc_begin(0, U, out=P)
    for mode in ("dense", "proj"):
        rc = eng.lib.cesx_gp_hmc_leap(eng._h, eng_mod.GP_MODES[mode], P.data_ptr(), *(r.data_ptr() for r in rows), None)
        assert rc == eng_mod.EINVAL
    assert np.all(same_bits(U.cpu().numpy(), Uh)) and np.all(same_bits(eng.mh_phi(), phi0))           # nothing was touched
    eng.gp_hmc_leap("proj", P, *rows)
    eng.gp_hmc_accept("proj", 0, U, P, *rows)
    assert eng.mh_stats()[0] == 1


# ---- end to end: gp_mh(chains=, pca_tools=, sigma_form='projected', update=) -----------------------------------------------

E2E_DELTA = 0.15              # accept rates 0.8 .. 0.95 on the host chains of both shapes, Langevin and L = 3 (NOTEBOOK.md)


def _mc(y, **attrs):
    from ces_amd import sample
    mc = sample.MCMC()
    mc.mute_bar = True
    mc.y_obs = y
    for key, val in attrs.items():
        setattr(mc, key, val)
    return mc


def host_chain(enka, prior, y, Gamma, pca, compounded, seed, steps, leapfrog):
    """One chain on the host from predict_gps(grad=True) on the k GPs and MCMC.langevin_phi_grad_pca, the draws per step the
    random walk's (xi, then u): (samples (p, steps + 1), margin and phi(current) per step, accept rate).  leapfrog None: the
    Langevin step."""
    from ces_amd import emulate
    from ces_amd.sample import MCMC
    state = np.random.get_state()
    np.random.seed(seed)
    p = enka.p
    scales = E2E_DELTA * np.linalg.cholesky(np.cov(enka.Ustar))

    def score(u):
        rows = emulate.predict_gps(enka, u.reshape(1, -1), grad=True)
        phi, grad = MCMC.langevin_phi_grad_pca(*rows, u.reshape(1, -1), y, Gamma, pca["VD_k"], pca["mG"], compounded,
                                               prior.mean, prior.cov)
        return phi[0], scales.T @ grad[0]
    cur = enka.Ustar.mean(axis=1)
    phi_c, g_c = score(cur)
    samples, margins, phis, acc = [cur], [], [], 0
    for _ in range(steps):
        xi = np.random.normal(0, 1, p)
        if leapfrog is None:
            prop = cur + scales @ (xi - 0.5 * g_c)
            phi_p, g_p = score(prop)
            corr = MCMC.langevin_correction(xi, g_c, g_p)
        else:
            prop, phi_p, g_p, r = MCMC.hmc_trajectory(score, scales, cur, g_c, xi, leapfrog)
            corr = 0.5 * (xi * xi).sum() - 0.5 * (r * r).sum()
        margin = phi_c - phi_p + corr - np.log(np.random.uniform())
        margins.append(margin)
        phis.append(phi_c)
        if margin > 0:
            cur, phi_c, g_c = prop, phi_p, g_p
            acc += 1
        samples.append(cur)
    np.random.set_state(state)
    return np.array(samples).T, np.array(margins), np.array(phis), acc / steps


@pytest.mark.parametrize("update,leapfrog", [("langevin", None), ("hmc", 3)])
@pytest.mark.parametrize("n,compounded", [(129, False), (180, True)])
def test_chains1_reproduces_the_host_chain(n, compounded, update, leapfrog):
    man, a = load_gold()
    prior = gold_prior(a)
    enka, y, Gamma, pca = stretched(a, n)
    steps, seed = 20, 4100 + n
    host, margins, phis, rate = host_chain(enka, prior, y, Gamma, pca, compounded, seed, steps, leapfrog)
    mc = _mc(y)
    np.random.seed(seed)
    extra = {} if leapfrog is None else dict(leapfrog=leapfrog)
    mc.gp_mh(enka, steps, prior, delta=E2E_DELTA, pca_tools=pca, Gamma=Gamma, noise_compounded=compounded, chains=1, start="mean",
             sigma_form="projected", update=update, **extra)
    assert mc.samples.shape == host.shape == (enka.p, steps + 1)
    off = np.any(np.abs(mc.samples - host) > 1e-9 * np.maximum(1.0, np.abs(host)), axis=0)
    if off.any():                      # a tie ends the comparison: the step before the first difference lay inside the band
        t = int(np.flatnonzero(off)[0]) - 1
        assert abs(margins[t]) <= sr.BAND * max(1.0, abs(phis[t])), (t, margins[t], phis[t])
    else:
        assert abs(mc.accept - rate) < 1e-12
    assert 0.0 < rate < 1.0


@pytest.mark.parametrize("update,leapfrog", [("langevin", None), ("hmc", 3)])
def test_33_chains_run_summarise_and_adapt(update, leapfrog):
    man, a = load_gold()
    enka, y, Gamma, pca = stretched(a, 180)
    extra = {} if leapfrog is None else dict(leapfrog=leapfrog)
    kw = dict(chains=33, pca_tools=pca, Gamma=Gamma, noise_compounded=True, sigma_form="projected", update=update, **extra)
    mc = _mc(y, noise="device", seed=77)
    mc.gp_mh(enka, 20, gold_prior(a), delta=E2E_DELTA, summary=True, autocorr=dict(lags=8), **kw)
    assert 0.0 < mc.accept < 1.0 and mc.accept_chains.shape == (33,)
    assert np.all(np.isfinite(mc.summary["mean"])) and mc.autocorr is not None
    # adapt=10 of 20 steps ends with a finite multiplier; a fresh sampler at the returned delta continues bit for bit
    X = _mc(y, noise="device", seed=77)
    X.gp_mh(enka, 20, gold_prior(a), delta=E2E_DELTA, adapt=10, **kw)
    assert np.isfinite(X.adapt["multiplier"]) and X.adapt["multiplier"] > 0 and X.samples.shape == (enka.p, 21, 33)
    Y = _mc(y, noise="device", seed=77)
    Y.samples, Y._mh_next_step = X.samples[:, :11, :].copy(), 10
    Y.gp_mh(enka, 10, gold_prior(a), delta=X.adapt["delta"], **kw)
    assert np.array_equal(Y.samples, X.samples) and X.accept == Y.accept
