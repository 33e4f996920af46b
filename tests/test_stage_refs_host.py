"""The references of oracle/stage_ref.py against what is already pinned, so that a wrong reference cannot pass a wrong
kernel: its accept step replays the chains of the real reference (tests/golden/mcmc.npz, gp_mcmc.npz) from the fixtures'
own draws, and its restatement of the device uniform equals a scalar restatement in Python integers that is itself held
to the Random123 known answers."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_emulate_host import gold_call, gold_prior, gold_problem, load_gold  # noqa: E402
from test_mcmc_host import load_cases, setup_case  # noqa: E402

from oracle import stage_ref as sr  # noqa: E402

M32 = 0xFFFFFFFF


def moves(samples):
    return np.any(np.diff(samples, axis=1) != 0, axis=0)


# ---- the accept reference against the reference's own chains -------------------------------------------------------

@pytest.mark.parametrize("case", [c["name"] for c, _ in load_cases()])
def test_accept_reference_replays_model_mh_fixtures(case):
    c, a = next((c, a) for c, a in load_cases() if c["name"] == case)
    _, _, enka, prior = setup_case(c, a)
    kw, p = c["kwargs"], c["p"]
    update, beta = kw.get("update"), kw.get("beta", 0.5)
    # the scales as ces/sample.py:122-129 forms them
    if kw.get("enka_scaling", True):
        scales = kw.get("delta", 1.0) * np.linalg.cholesky(np.cov(enka.Ustar).reshape(p, p))
    else:
        scales = kw.get("delta", 1.0) * np.eye(p)
    if update == "pCN":
        scales = np.linalg.cholesky(prior.cov)
    # whitened data rows with unit weights (a dense Gamma among the cases); the prior rows w = L_Sigma^{-1} (x - mu)
    Lg = np.linalg.cholesky(a["Gamma"])
    yw, gw = np.linalg.solve(Lg, a["y"]), np.ones(c["n_obs"])

    def phi(X):
        rows = None if update == "pCN" else sr.dense_prior_rows(X, a["mu"], a["Sigma"])
        return sr.mh_phi(np.linalg.solve(Lg, a["A"] @ X), yw, gw, rows)

    cur = enka.Ustar.mean(axis=1).reshape(p, 1)
    ref = sr.AcceptRef(phi(cur))
    phi_start = ref.phi.copy()
    samples = [cur[:, 0].copy()]
    accepted_since = 0
    np.random.seed(c["seed"])
    for k in range(c["steps"]):
        if c["resume"] and k == c["resume"]:
            ref.phi = phi_start.copy()              # the reference's resume keeps phi of the start point (:131-163)
            accepted_since = 0
        xi = np.random.normal(0, 1, p)
        logu = np.log(np.random.uniform())
        P = sr.propose(cur, scales, xi[:, None], update, beta)
        pp = phi(P)
        acc, band = ref.decide(pp, [logu])
        ref.commit(acc, pp, band)
        if acc[0]:
            cur = P
            accepted_since += 1
        samples.append(cur[:, 0].copy())
    got = np.array(samples).T
    assert np.array_equal(moves(got), moves(a["samples"]))
    np.testing.assert_allclose(got, a["samples"], rtol=1e-12, atol=1e-12)
    assert ref.left_out == 0 and ref.chain_steps == c["steps"]
    assert int(ref.count[0]) == int(moves(a["samples"]).sum())
    assert accepted_since / (c["steps"] - c["resume"]) == pytest.approx(float(a["accept"]), abs=1e-12)


GP_CASES = [c["name"] for c in load_gold()[0]["cases"] if c["name"] not in ("pca", "compounded_dense")]


@pytest.mark.parametrize("case", GP_CASES)
def test_accept_reference_replays_gp_mh_fixtures(case):
    from ces_amd import emulate as em
    man, a = load_gold()
    c = [c for c in man["cases"] if c["name"] == case][0]
    enka = gold_problem(a, c["scaled"])
    prior = gold_prior(a)
    call = gold_call(a, c["kwargs"])
    p, n = enka.p, enka.n_obs
    Gamma = call.get("Gamma")
    mode = "var" if Gamma is None else ("gamma_var" if call.get("noise_compounded") else "gamma")
    Gamma = np.eye(n) if Gamma is None else Gamma
    if call.get("enka_scaling", True):
        scales = call.get("delta", 1.0) * np.linalg.cholesky(np.cov(enka.Ustar))
    else:
        scales = call.get("delta", 1.0) * np.eye(p)

    def phi(X):
        mean, var = em.predict_gps(enka, X.T, nugget=call.get("nugget", True))
        return sr.gp_phi(mode, mean, var, a["prob_y"], Gamma, X, prior.mean, prior.cov)

    cur = enka.Ustar.mean(axis=1).reshape(p, 1)
    ref = sr.AcceptRef(phi(cur))
    samples = [cur[:, 0].copy()]
    np.random.seed(c["seed"])
    for k in range(man["STEPS"]):
        xi = np.random.normal(0, 1, p)
        logu = np.log(np.random.uniform())
        P = sr.propose(cur, scales, xi[:, None], call.get("update"), call.get("beta", 0.5))
        pp = phi(P)
        acc, band = ref.decide(pp, [logu])
        ref.commit(acc, pp, band)
        if acc[0]:
            cur = P
        samples.append(cur[:, 0].copy())
    want = a["mh_%s_samples" % case]
    got = np.array(samples).T
    assert np.array_equal(moves(got), moves(want))
    np.testing.assert_allclose(got, want, rtol=1e-10, atol=1e-10)
    assert ref.left_out == 0
    assert int(ref.count[0]) == int(moves(want).sum())


def test_a_non_positive_variance_scores_as_a_rejection():
    rng = np.random.default_rng(0)
    n, p, M = 3, 2, 6
    mean, var = rng.standard_normal((n, M)), 0.5 + rng.random((n, M))
    var[1, 1], var[2, 2], var[0, 3], mean[0, 3] = -0.25, 0.0, 0.0, 0.7
    y = np.array([0.1, 0.2, 0.7])                       # (d = 0 where var[0, 3] = 0)
    X = rng.standard_normal((p, M))
    for mode, Gamma in (("var", np.eye(n)), ("gamma_var", np.zeros((n, n)))):
        ph = sr.gp_phi(mode, mean, var, y, Gamma, X, np.zeros(p), np.eye(p))
        assert np.array_equal(np.isinf(ph), [False, True, True, True, False, False])
        ref = sr.AcceptRef(np.full(M, 1e6))
        acc, band = ref.decide(ph, np.full(M, -1e-3))
        assert np.array_equal(acc, ~np.isinf(ph)) and not band.any()


def test_the_band_and_the_cap():
    ref = sr.AcceptRef(np.array([100.0, 100.0, 0.5, 0.5]))
    # margins 5e-8 (inside 1e-9 x 100), 2e-7 (outside), 5e-10 (inside 1e-9 x 1), -2e-9 (outside)
    phi_p = np.array([99.0, 99.0, 0.25, 0.25])
    logu = np.array([1.0 - 5e-8, 1.0 - 2e-7, 0.25 - 5e-10, 0.25 + 2e-9])
    acc, band = ref.decide(phi_p, logu)
    assert np.array_equal(band, [True, False, True, False]) and np.array_equal(acc, [True, True, True, False])
    ref.commit([False, True, True, False], phi_p, band)          # (the device's decision for the chains in the band)
    assert np.array_equal(ref.phi, [100.0, 99.0, 0.25, 0.5]) and np.array_equal(ref.count, [0, 1, 1, 0])
    assert ref.left_out == 2 and ref.chain_steps == 4 and not ref.within_cap()
    ref.chain_steps = 2000
    assert ref.within_cap()
    _, band = ref.decide(phi_p, logu, half_width=0.0)
    assert not band.any()


# ---- the proposal --------------------------------------------------------------------------------------------------

def test_propose_is_the_samplers_step():
    from ces_amd import sample
    mc = sample.MCMC()
    S = np.array([[2.0, 0.0, 0.0], [0.5, 1.0, 0.0], [-0.3, 0.2, 0.7]])
    u = np.array([1.0, -1.0, 0.25])
    for update, step in ((None, lambda: mc.random_walk(u, S, 3)), ("pCN", lambda: mc.pCN(u, S, 3, beta=0.3))):
        np.random.seed(3)
        want = step()
        np.random.seed(3)
        xi = np.random.normal(0, 1, 3)
        got = sr.propose(u[:, None], S, xi[:, None], update, 0.3)[:, 0]
        np.testing.assert_allclose(got, want, rtol=1e-15, atol=0)


def test_mh_noise_is_the_noise_block_of_the_mh_step_word():
    from oracle import philox
    a = sr.mh_noise(5, 7, 0x1234567890, 3, 11, np.float64)
    assert np.array_equal(a, philox.noise_block(5, 7, 0x1234567890, 3 | 2 ** 31, 11, np.float64))
    assert not np.array_equal(a, philox.noise_block(5, 7, 0x1234567890, 3, 11, np.float64))
    assert sr.mh_step_word(0) == 2 ** 31 and sr.mh_step_word(2 ** 31 - 1) == M32


# ---- the uniform ---------------------------------------------------------------------------------------------------

def philox_int(ctr, key):
    """Philox4x32-10 in Python integers (Salmon et al., SC'11), written apart from oracle/philox.py."""
    c0, c1, c2, c3 = ctr
    k0, k1 = key
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def log_uniform_int(gj, seed, step):
    x, y, _, _ = philox_int((gj & M32, gj >> 32, M32, step | 2 ** 31), (seed & M32, seed >> 32))
    m53 = ((x >> 5) << 26) | (y >> 6)
    return math.log((m53 + 0.5) * 2.0 ** -53)


def test_the_scalar_restatement_meets_the_random123_known_answers():
    assert philox_int((0, 0, 0, 0), (0, 0)) == (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)
    assert philox_int((M32,) * 4, (M32, M32)) == (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)
    assert philox_int((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0)) == \
        (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)


def test_log_uniform_equals_the_scalar_restatement():
    seed = 0x9E3779B97F4A7C15
    for j_offset in (0, 2 ** 32 + 7):
        for step in (0, 1, 12345, 2 ** 31 - 1):
            lu = sr.log_uniform(40, seed, step, j_offset)
            for j in (0, 1, 2, 17, 39):
                want = log_uniform_int(j_offset + j, seed, step)
                assert abs(lu[j] - want) <= 4e-16 * abs(want), (j_offset, step, j)


def test_log_uniform_is_a_log_of_an_open_unit_interval_and_moves_with_every_counter_word():
    seed = 0xABCDEF0123456789
    base = sr.log_uniform(4096, seed, 5)
    assert np.all(np.isfinite(base)) and np.all(base < 0.0)
    u = np.exp(base)
    assert abs(u.mean() - 0.5) < 0.02 and abs(u.var() - 1.0 / 12.0) < 0.01
    assert len(np.unique(base)) == base.size                               # chains differ
    others = [sr.log_uniform(4096, seed, 6), sr.log_uniform(4096, seed + 1, 5), sr.log_uniform(4096, seed + 2 ** 32, 5),
              sr.log_uniform(4096, seed, 5, j_offset=2 ** 32)]
    for other in others:                                                   # steps, both seed words, the high index word
        assert not np.any(other == base)
    assert np.array_equal(sr.log_uniform(4096, seed, 5, j_offset=100)[:-100], base[100:])
    # (its own counter domain: not the first uniform of any xi row quad of the same chain and step)
    from oracle import philox
    j = np.arange(8, dtype=np.uint32)
    z = np.zeros(8, dtype=np.uint32)
    x, y, _, _ = philox.philox4x32_10(j, z, z, np.full(8, 5 | 2 ** 31, dtype=np.uint32), seed & M32, seed >> 32)
    m53 = ((x.astype(np.uint64) >> np.uint64(5)) << np.uint64(26)) | (y.astype(np.uint64) >> np.uint64(6))
    assert not np.any(np.log((m53 + 0.5) * 2.0 ** -53) == base[:8])
