"""The dense per-chain likelihood of gp_mh(chains=, pca_tools=) on the host (no device): the bar of tests/gp_dense_cases.py
holds for a numpy restatement of gp_score_dense_kernel's order and bites on six deliberately wrong kernels; the argument
checks of the Python route; the two new entry points in the binding's export list."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gp_dense_cases as gc  # noqa: E402
from test_emulate_host import gold_prior, gold_problem, load_gold  # noqa: E402

from oracle import stage_ref as sr  # noqa: E402

CASE_IDS = ["%s-n%d-k%d" % (kind, n, k) for n, k, _, kind in gc.HOST_CASES]


def _case(n, k, cg, kind, variant):
    logdet, dense_prior = bool(variant & 1), bool(variant & 2)
    rng = np.random.default_rng([n, k, int(cg), kind == "pca", variant])
    pr = gc.problem(rng, n, k, cg, kind, dense_prior=dense_prior)
    m, v = gc.rows(rng, k, gc.HOST_M)
    X = gc.states(rng, pr, gc.HOST_M)
    return pr, m, v, X, logdet


def test_the_case_tables_cover_what_they_must():
    assert len(gc.HOST_CASES) == 14 and {c[0] for c in gc.HOST_CASES} == {1, 2, 7, 50, 63, 64, 65, 96, 128}
    assert {c[3] for c in gc.HOST_CASES} == set(gc.FAMILIES)
    assert all(1 <= k <= n <= gc.NMAX for n, k, _, _ in gc.HOST_CASES)
    assert {n for n, _ in gc.GPU_SHAPES} == {1, 2, 63, 64, 65, 127, 128}
    for n in gc.GPU_N:
        assert {k for nn, k in gc.GPU_SHAPES if nn == n} == {k for k in (1, 3, n) if k <= n}


@pytest.mark.parametrize("case", gc.HOST_CASES, ids=CASE_IDS)
def test_the_kernels_order_stays_within_the_bound(case):
    n, k, cg, kind = case
    for variant in (1, 2):                                   # (log det, diagonal prior) and (none, dense prior)
        pr, m, v, X, logdet = _case(n, k, cg, kind, variant)
        phi, bound, cond, q = gc.reference(pr, m, v, X, logdet)
        assert np.all(cond <= gc.COND_SCORE), cond.max()
        got = gc.kernel_order(pr, m, v, X, logdet)
        ratio = np.abs(got - phi) / bound
        print("n=%d k=%d %s logdet=%d: cond_2 up to %.1e, worst |phi - ref| / bound %.3g" % (n, k, kind, logdet, cond.max(), ratio.max()))
        assert np.all(np.abs(got - phi) <= bound), (variant, ratio.max())


@pytest.mark.parametrize("case", gc.HOST_CASES, ids=CASE_IDS)
def test_every_mutant_leaves_four_bounds(case):
    """(a NaN where the reference is finite has left the bound too)"""
    n, k, cg, kind = case
    variant = 1 + 2 * (n % 2)                                # the log det term; the prior alternates over the cases
    pr, m, v, X, logdet = _case(n, k, cg, kind, variant)
    phi, bound, _, _ = gc.reference(pr, m, v, X, logdet)
    shown = 0
    for mutant in gc.MUTANTS:
        if gc.mutant_is_identity(mutant, n, k, kind, logdet):
            continue
        got = gc.kernel_order(pr, m, v, X, logdet, mutant)
        with np.errstate(invalid="ignore"):
            left = ~(np.abs(got - phi) <= 4 * bound)
        assert left.any(), (mutant, float(np.nanmax(np.abs(got - phi) / bound)))
        shown += 1
    assert shown >= 4


def test_every_mutant_shows_in_every_family():
    for kind in gc.FAMILIES:
        for mutant in gc.MUTANTS:
            live = [c for c in gc.HOST_CASES if c[3] == kind and not gc.mutant_is_identity(mutant, c[0], c[1], kind, True)]
            assert live or (mutant == "diagonal" and kind == "cmp"), (kind, mutant)      # (B = I: B diag(v) B^T IS its diagonal)


ACCEPT_CASES = [(7, 3, "pca"), (65, 5, "pca"), (128, 16, "pca"), (50, 50, "cmp")]


@pytest.mark.parametrize("n,k,kind", ACCEPT_CASES)
def test_the_accept_loop_leaves_out_nothing(n, k, kind):
    """8 steps of 24 chains: the decisions of the kernel's order equal the reference's on every chain-step, and no
    chain-step lies within the band max(1e-9 max(1, |phi|), bound(U) + bound(P)) of a tie (the seeds are fixed so that
    the reference alone leaves out none: its count does not depend on the code under test)."""
    M, steps = gc.HOST_M, 8
    rng = np.random.default_rng([n, k, kind == "pca", 77])
    pr = gc.problem(rng, n, k, 1e2, kind, dense_prior=n % 2 == 0, b_scale=(-2.0, 0.0))
    S = 0.3 * np.linalg.cholesky(pr["Sp"])
    U = gc.states(rng, pr, M)
    m, v = gc.rows(rng, k, M, v_lo=1e-6)
    phi0, b0, cond, _ = gc.reference(pr, m, v, U, True)
    assert np.all(cond <= gc.COND_ACCEPT)
    ref = gc.DenseAcceptRef(phi0, b0)
    mine = gc.kernel_order(pr, m, v, U, True)
    for step in range(steps):
        P = sr.propose(U, S, rng.standard_normal((pr["p"], M)))
        m, v = gc.rows(rng, k, M, v_lo=1e-6)
        logu = np.log(rng.random(M))
        phi_p, b_p, cond, _ = gc.reference(pr, m, v, P, True)
        assert np.all(cond <= gc.COND_ACCEPT)
        acc, band = ref.decide(phi_p, logu, ref.half_width(b_p))
        mine_p = gc.kernel_order(pr, m, v, P, True)
        took = logu < mine - mine_p
        assert not band.any(), (step, np.flatnonzero(band))
        assert np.array_equal(took, acc), (step, np.flatnonzero(took != acc))
        ref.commit(acc, phi_p, band)
        mine = np.where(took, mine_p, mine)
        U = np.where(acc[None, :], P, U)
    assert ref.left_out == 0 and ref.chain_steps == steps * M
    assert 0 < ref.count.sum() < steps * M


def test_the_constant_of_the_bound_covers_the_references_own_error():
    """The measurement behind the 16, on the shapes up to n = 65 with 4 chains each (the 80-bit Cholesky is a Python loop):
    both fp64 paths against the long-double truth, in units of cond_2 eps q and of n eps (cond_2)."""
    small = [c for c in gc.MEASURE_CASES if c[0] <= 65]
    w = gc.measure_reference_error(small, M=4)
    print("worst ratios: chol quad %.3g, LU-reference quad %.3g (of cond eps q); chol log det %.3g of n eps; eigvals %.3g of n eps cond" % tuple(w))
    assert w[0] < 16 and w[1] < 16 and w[3] < 16


def _mc(a):
    from ces_amd import sample
    mc = sample.MCMC()
    mc.mute_bar = True
    mc.y_obs = a["prob_y"]
    return mc


def test_gp_mh_pca_argument_checks():
    man, a = load_gold()
    enka = gold_problem(a)
    prior = gold_prior(a)
    pca = dict(VD_k=a["prob_VD_k"], mG=a["prob_mG"])
    with pytest.raises(ValueError, match="pca_tools"):                        # the reference cannot run this either
        _mc(a).gp_mh(enka, 2, prior, chains=4, pca_tools=pca)
    with pytest.raises(ValueError, match="VD_k"):                            # rows != n_obs
        _mc(a).gp_mh(enka, 2, prior, chains=4, Gamma=a["prob_Gamma_dense"], pca_tools=dict(VD_k=a["prob_VD_k"][:3], mG=a["prob_mG"]))
    with pytest.raises(ValueError, match="mG"):
        _mc(a).gp_mh(enka, 2, prior, chains=4, Gamma=a["prob_Gamma_dense"], pca_tools=dict(VD_k=a["prob_VD_k"], mG=a["prob_mG"][:3]))
    with pytest.raises(ValueError, match="3 GPs for the k = 4"):             # len(gpmodels) != k
        _mc(a).gp_mh(enka, 2, prior, chains=4, Gamma=a["prob_Gamma_dense"], pca_tools=pca, gpmodels=enka.gpmodels[:3])
    with pytest.raises(ValueError, match="2 columns|k = 2"):
        _mc(a).gp_mh(enka, 2, prior, chains=4, Gamma=a["prob_Gamma_dense"],
                     pca_tools=dict(VD_k=a["prob_VD_k"][:, :2], mG=a["prob_mG"]))
    with pytest.raises(ValueError, match="separable"):
        _mc(a).gp_mh(enka, 2, prior, chains=4, Gamma=a["prob_Gamma_dense"], pca_tools=pca, separable=True)


def test_gp_mh_pca_names_the_limit_at_n_129():
    from test_emulate_host import Enka
    man, a = load_gold()
    enka = gold_problem(a)
    big = Enka(enka.p, 129, enka.Ustar, np.zeros((129, enka.Ustar.shape[1])))
    big.gpmodels = enka.gpmodels
    mc = _mc(a)
    mc.y_obs = np.zeros(129)
    with pytest.raises(ValueError, match="128"):
        mc.gp_mh(big, 2, gold_prior(a), chains=4, Gamma=np.eye(129), pca_tools=dict(VD_k=np.eye(129)[:, :4], mG=np.zeros(129)))


def test_the_new_entry_points_are_exported():
    from ces_amd import engine
    assert "cesx_gp_dense_set" in engine.EXPORTS and "cesx_mh_phi" in engine.EXPORTS
    assert engine.GP_MODES["dense"] == 3 and engine.GP_DENSE_NMAX == gc.NMAX
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "cesx.h")) as fh:
        hdr = fh.read()
    assert "#define CESX_GP_DENSE      3" in hdr and "#define CESX_GP_DENSE_NMAX %d" % gc.NMAX in hdr
    assert "#define CESX_ABI_VERSION %d" % engine.ABI_VERSION in hdr and engine.ABI_VERSION >= 4
    import ctypes
    assert ctypes.sizeof(engine.GpDenseDesc) == 4 * 3 + 4 + 8 * 2        # 3 x 32-bit + pad, 2 pointers
