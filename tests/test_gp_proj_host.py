"""The projected per-chain likelihood of gp_mh(chains=, pca_tools=, sigma_form='projected') on the host (no device): the bar
of tests/gp_proj_cases.py holds for a numpy restatement of gp_score_proj_kernel's order and bites on five deliberately wrong
kernels; the host reduction reassembles Sigma; the argument checks of the Python route; header and binding; the stage
struct's ownership in a stand-alone host program.

Worst |phi - reference| / bound_j is printed (pytest -s) and recorded in NOTEBOOK.md."""
import ctypes
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gp_dense_cases as gc  # noqa: E402
import gp_proj_cases as gq  # noqa: E402
from test_emulate_host import Enka, gold_prior, gold_problem, load_gold  # noqa: E402

from oracle import stage_ref as sr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE_IDS = ["n%d-k%d" % s for s in gq.HOST_SHAPES]


def _case(n, k, variant, b_scale=(-2.0, 1.0)):
    logdet, dense_prior = bool(variant & 1), bool(variant & 2)
    rng = np.random.default_rng([n, k, variant, int(b_scale[1])])
    pr = gc.problem(rng, n, k, gq.cond_gamma_of(n), "pca", dense_prior=dense_prior, b_scale=b_scale)
    m, v = gc.rows(rng, k, gq.HOST_M)
    X = gc.states(rng, pr, gq.HOST_M)
    return pr, m, v, X, logdet


def test_the_case_tables_cover_what_they_must():
    assert set(gq.HOST_SHAPES) == {(1, 1), (7, 3), (50, 8), (128, 16), (129, 4), (180, 16), (180, 128), (300, 64), (65, 65)}
    assert gq.BIG_B == (180, 16, (2.0, 5.0))
    from ces_amd import engine
    assert gq.GPU_K == [1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128] and max(gq.GPU_K) == gq.KMAX == engine.GP_PROJ_KMAX
    assert all(n == max(k, 129) for n, k in gq.GPU_SHAPES[:len(gq.GPU_K)]) and gq.GPU_SHAPES[-2:] == [(180, 16), (300, 64)]
    assert len(gq.MUTANTS) == 5


WORST = {"ratio": 0.0}


def _hold(pr, m, v, X, logdet, label, cond_cap):
    phi, bound, cond, q, cond_s = gq.reference(pr, m, v, X, logdet)
    if cond_cap is not None:
        assert np.all(cond_s <= cond_cap), cond_s.max()
    got = gq.kernel_order_proj(pr, m, v, X, logdet)
    ratio = np.abs(got - phi) / bound
    WORST["ratio"] = max(WORST["ratio"], float(ratio.max()))
    print("%s logdet=%d: cond_2(Sigma) up to %.1e, worst |phi - ref| / bound %.3g (so far %.3g)"
          % (label, logdet, cond_s.max(), ratio.max(), WORST["ratio"]))
    assert np.all(np.abs(got - phi) <= bound), (label, ratio.max())


@pytest.mark.parametrize("shape", gq.HOST_SHAPES, ids=CASE_IDS)
def test_the_kernels_order_stays_within_the_bound(shape):
    n, k = shape
    for variant in (1, 2):                                   # (log det, diagonal prior) and (none, dense prior)
        pr, m, v, X, logdet = _case(n, k, variant)
        _hold(pr, m, v, X, logdet, "n=%d k=%d" % (n, k), gc.COND_SCORE)


def test_the_bound_holds_where_b_diag_v_bt_dwarfs_gamma():
    """b_scale = (2, 5) at (180, 16): B diag(v) B^T >> Gamma, cond_2(Sigma_j) far past COND_SCORE -- this family is EXEMPT from
    the COND_SCORE assert (the bound carries cond_2 itself); it is the regime in which a Woodbury form subtracts two large
    numbers and this one does not."""
    n, k, b_scale = gq.BIG_B
    for variant in (1, 2):
        pr, m, v, X, logdet = _case(n, k, variant, b_scale)
        assert np.linalg.eigvalsh((pr["B"] * v.max(axis=1)) @ pr["B"].T).max() > 1e3 * np.linalg.eigvalsh(pr["Gamma"]).max()
        _hold(pr, m, v, X, logdet, "n=%d k=%d b_scale=(2, 5)" % (n, k), None)


MUTANT_CASES = [(n, k, (-2.0, 1.0)) for n, k in gq.HOST_SHAPES] + [gq.BIG_B]


@pytest.mark.parametrize("n,k,b_scale", MUTANT_CASES, ids=CASE_IDS + ["n180-k16-bigB"])
def test_every_mutant_leaves_four_bounds(n, k, b_scale):
    """(a NaN where the reference is finite has left the bound too)"""
    variant = 1 + 2 * (n % 2)                                # the log det term; the prior alternates over the cases
    pr, m, v, X, logdet = _case(n, k, variant, b_scale)
    phi, bound, _, _, _ = gq.reference(pr, m, v, X, logdet)
    proj = gq.project(pr)
    shown = 0
    for mutant in gq.MUTANTS:
        if gq.mutant_is_identity(mutant, n, k, logdet):
            continue
        got = gq.kernel_order_proj(pr, m, v, X, logdet, mutant, proj)
        with np.errstate(invalid="ignore"):
            left = ~(np.abs(got - phi) <= 4 * bound)
        assert left.any(), (mutant, float(np.nanmax(np.abs(got - phi) / bound)))
        shown += 1
    assert shown >= 4


def test_project_sigma_reassembles_sigma():
    """L (I + Q S Q^T) L^T = Sigma to rounding at n = 180, with Q = W R^{-1} recovered from the returned R; the two scalars
    and a0 give the literal quadratic form and log det."""
    from ces_amd import emulate
    n, k = 180, 16
    rng = np.random.default_rng([n, k, 5])
    pr = gc.problem(rng, n, k, 1e4, "pca")
    m, v = gc.rows(rng, k, 1)
    m, v = m[:, 0], v[:, 0]
    R, a0, c_perp, hld = emulate.project_sigma(pr["Gamma"], pr["B"], pr["g0"], pr["y"])
    assert R.shape == (k, k) and np.array_equal(R, np.triu(R)) and a0.shape == (k,) and c_perp >= 0.0
    L = np.linalg.cholesky(pr["Gamma"])
    W = np.linalg.solve(L, pr["B"])
    Q = np.linalg.solve(R.T, W.T).T
    assert np.abs(Q.T @ Q - np.eye(k)).max() < 1e-9
    S = (R * v) @ R.T
    Sig = gc.sigma_of(pr, v)
    back = L @ (np.eye(n) + Q @ S @ Q.T) @ L.T
    assert np.abs(back - Sig).max() <= 1e-10 * np.abs(Sig).max()
    d = pr["B"] @ m + pr["g0"] - pr["y"]
    a = a0 + R @ m
    quad = c_perp + a @ np.linalg.solve(np.eye(k) + S, a)
    want = d @ np.linalg.solve(Sig, d)
    assert abs(quad - want) <= 1e-8 * abs(want)
    assert abs(2 * hld + np.linalg.slogdet(np.eye(k) + S)[1] - np.linalg.slogdet(Sig)[1]) <= 1e-9 * n
    # rank-deficient VD_k: no special case
    B2 = pr["B"].copy()
    B2[:, 1] = B2[:, 0]
    R2, a2, c2, _ = emulate.project_sigma(pr["Gamma"], B2, pr["g0"], pr["y"])
    S2 = (R2 * v) @ R2.T
    a = a2 + R2 @ m
    d = B2 @ m + pr["g0"] - pr["y"]
    want = d @ np.linalg.solve(pr["Gamma"] + (B2 * v) @ B2.T, d)
    assert abs(c2 + a @ np.linalg.solve(np.eye(k) + S2, a) - want) <= 1e-8 * abs(want)
    with pytest.raises(ValueError, match="positive definite"):
        emulate.project_sigma(-pr["Gamma"], pr["B"], pr["g0"], pr["y"])
    with pytest.raises(ValueError, match="non-finite"):
        emulate.project_sigma(pr["Gamma"], pr["B"], pr["g0"], np.where(np.arange(n) == 3, np.nan, pr["y"]))


ACCEPT_SHAPES = [(129, 4), (180, 16), (300, 33), (180, 128)]


@pytest.mark.parametrize("n,k", ACCEPT_SHAPES)
def test_the_accept_loop_leaves_out_nothing(n, k):
    """8 steps of 24 chains: the decisions of the kernel's order equal the reference's on every chain-step, and no chain-step
    lies within the band max(1e-9 max(1, |phi|), bound(U) + bound(P)) of a tie (the seeds are fixed so that the reference
    alone leaves out none: its count does not depend on the code under test)."""
    M, steps = gq.HOST_M, 8
    rng = np.random.default_rng([n, k, 77])
    pr = gc.problem(rng, n, k, 1e2, "pca", dense_prior=n % 2 == 0, b_scale=(-2.0, 0.0))
    proj = gq.project(pr)
    S = 0.3 * np.linalg.cholesky(pr["Sp"])
    U = gc.states(rng, pr, M)
    m, v = gc.rows(rng, k, M, v_lo=1e-6)
    phi0, b0, cond, _, _ = gq.reference(pr, m, v, U, True)
    assert np.all(cond <= 1e4)
    ref = gc.DenseAcceptRef(phi0, b0)
    mine = gq.kernel_order_proj(pr, m, v, U, True, proj=proj)
    for step in range(steps):
        P = sr.propose(U, S, rng.standard_normal((pr["p"], M)))
        m, v = gc.rows(rng, k, M, v_lo=1e-6)
        logu = np.log(rng.random(M))
        phi_p, b_p, cond, _, _ = gq.reference(pr, m, v, P, True)
        assert np.all(cond <= 1e4)
        acc, band = ref.decide(phi_p, logu, ref.half_width(b_p))
        mine_p = gq.kernel_order_proj(pr, m, v, P, True, proj=proj)
        took = logu < mine - mine_p
        assert not band.any(), (step, np.flatnonzero(band))
        assert np.array_equal(took, acc), (step, np.flatnonzero(took != acc))
        ref.commit(acc, phi_p, band)
        mine = np.where(took, mine_p, mine)
        U = np.where(acc[None, :], P, U)
    assert ref.left_out == 0 and ref.chain_steps == steps * M
    assert 0 < ref.count.sum() < steps * M


def _mc(a, n=None):
    from ces_amd import sample
    mc = sample.MCMC()
    mc.mute_bar = True
    mc.y_obs = a["prob_y"] if n is None else np.zeros(n)
    return mc


def _stretched(enka, n, n_gp=None):
    big = Enka(enka.p, n, enka.Ustar, np.zeros((n, enka.Ustar.shape[1])))
    big.gpmodels = enka.gpmodels if n_gp is None else (list(enka.gpmodels) * n_gp)[:n_gp]
    return big


def test_gp_mh_sigma_form_argument_checks():
    man, a = load_gold()
    enka, prior = gold_problem(a), gold_prior(a)
    pca = dict(VD_k=a["prob_VD_k"], mG=a["prob_mG"])
    with pytest.raises(ValueError, match="sigma_form"):
        _mc(a).gp_mh(enka, 2, prior, chains=4, Gamma=a["prob_Gamma_dense"], pca_tools=pca, sigma_form="bogus")
    with pytest.raises(ValueError, match="chains"):                          # the host path has one form
        _mc(a).gp_mh(enka, 2, prior, Gamma=a["prob_Gamma_dense"], pca_tools=pca, sigma_form="projected")
    with pytest.raises(ValueError, match="pca_tools"):
        _mc(a).gp_mh(enka, 2, prior, chains=4, Gamma=a["prob_Gamma_dense"], sigma_form="projected")
    with pytest.raises(ValueError, match="pca_tools"):                        # ... and Gamma, as in the dense form
        _mc(a).gp_mh(enka, 2, prior, chains=4, pca_tools=pca, sigma_form="projected")
    n = 130
    with pytest.raises(ValueError, match="k <= 128"):
        _mc(a, n).gp_mh(_stretched(enka, n, 129), 2, prior, chains=4, Gamma=np.eye(n), sigma_form="projected",
                        pca_tools=dict(VD_k=np.eye(n)[:, :129], mG=np.zeros(n)))
    # n_obs = 129 without the kwarg raises as before, and now says where to go
    with pytest.raises(ValueError, match="128.*sigma_form='projected'"):
        _mc(a, 129).gp_mh(_stretched(enka, 129), 2, prior, chains=4, Gamma=np.eye(129),
                          pca_tools=dict(VD_k=np.eye(129)[:, :4], mG=np.zeros(129)))


def test_header_and_binding():
    from ces_amd import engine
    assert "cesx_gp_proj_set" in engine.EXPORTS and "cesx_gp_dense_set" in engine.EXPORTS
    assert engine.GP_MODES["proj"] == 4 and engine.GP_MODES["dense"] == 3 and engine.GP_PROJ_KMAX == gq.KMAX == 128
    with open(os.path.join(ROOT, "include", "cesx.h")) as fh:
        hdr = fh.read()
    assert "#define CESX_GP_PROJ       4" in hdr and "#define CESX_GP_PROJ_KMAX 128" in hdr
    assert "#define CESX_ABI_VERSION %d" % engine.ABI_VERSION in hdr and engine.ABI_VERSION >= 5
    assert "int cesx_gp_proj_set(cesx_handle h, const cesx_gp_proj_desc* desc);" in hdr
    assert ctypes.sizeof(engine.GpProjDesc) == 4 * 3 + 4 + 8 * 2 + 8 * 2     # 3 x 32-bit + pad, 2 pointers, 2 doubles
    assert [f[0] for f in engine.GpProjDesc._fields_] == ["struct_bytes", "k", "logdet", "R", "a0", "c_perp", "half_logdet_gamma"]


def test_the_proj_stage_struct_frees_what_it_owns(tmp_path):
    """tools/devbuf_check_proj.cpp: GpProjState over a malloc-backed dev_alloc / dev_free whose calls fail in turn, built with
    the host compiler alone (no ROCm include path)."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "devbuf_check_proj")
    build = subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tools", "devbuf_check_proj.cpp")],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    lines = run.stdout.splitlines()
    assert sum(ln.startswith("ok GpProjState:") for ln in lines) == 5, run.stdout
    assert not any(ln.startswith("FAILED") for ln in lines)
    assert lines[-1] == "5 scenarios, all ok"
