"""The Emulate stage at its ragged and strided edges: gp_score_kernel against the fp64 reference of oracle/stage_ref.py
on synthetic GP rows (every likelihood mode, a dense Gamma, a dense Sigma, v <= 0), gp_predict_kernel at the shapes where
its panel moves from LDS to the strided global workspace and where its block loops have remainders, and the gpfit
kernels at p > 8 (a second pass of the lengthscale sums), at tile edges and on coincident training inputs.

No bar is new: ties of the accept step are the band of tests/test_gpu_sample_edges.py (1e-9 max(1, |phi|), at most 1
chain-step in 1000 left out), the prediction keeps the bars of tests/test_gpu_gp.py (1e-9 of sum |alpha_j k_j| for the
mean, 1e-9 sigma^2 for the variance) and the fit the bar max(1e-9, 100 delta) of tests/test_gpu_gpfit.py."""
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_emulate_host import Enka, build_gps  # noqa: E402
from test_gpu_gp import FAMILIES, device_predict, np_predict, random_gps  # noqa: E402
from test_gpu_gpfit import IDX, _engine, _host_and_delta, _model, _problem, _thetas  # noqa: E402
from test_gpu_sample_edges import (SEED, STEPS, UNIFORM_STEPS, eng_mod, guarded, guards_intact, note, put,  # noqa: E402,F401
                                   run_accept_steps, same_bits)

from oracle import stage_ref as sr  # noqa: E402

pytestmark = pytest.mark.gpu


# ---- C. gp_score_kernel against fp64 -------------------------------------------------------------------------------------

GP_MODES = ["gamma", "gamma_dense", "var", "gamma_var"]          # 'gamma_dense': mode gamma with a dense (whitened) Gamma
SCORE_SHAPES = [(1, 1), (2, 4), (8, 32), (20, 33)]
SCORE_M = [3, 257, 1023]


def _score_cases():
    """Every (mode, prior, shape, dtype); the update and the chain count cycle so that every mode meets both updates and
    every chain count, and every shape every chain count."""
    cases = []
    for i, (mode, dense_sigma, (p, n)) in enumerate(itertools.product(GP_MODES, [False, True], SCORE_SHAPES)):
        for k, dtype in enumerate(("float64", "float32")):
            cases.append((mode, dense_sigma, p, n, SCORE_M[(i + i // 4 + k) % 3], dtype, [None, "pCN"][(i // 4 + i + k) % 2]))
    return cases


SCORE_CASES = _score_cases()


def test_the_score_cases_cover_what_they_must():
    assert len(SCORE_CASES) == 64 and len(set(SCORE_CASES)) == 64
    for mode in GP_MODES:
        mine = [c for c in SCORE_CASES if c[0] == mode]
        assert {c[6] for c in mine} == {None, "pCN"} and {c[4] for c in mine} == set(SCORE_M)
        assert {c[1] for c in mine} == {False, True} and {c[5] for c in mine} == {"float64", "float32"}
        assert {(c[2], c[3]) for c in mine} == set(SCORE_SHAPES)
    for shape in SCORE_SHAPES:
        assert {c[4] for c in SCORE_CASES if (c[2], c[3]) == shape} == set(SCORE_M)
    for kind in (None, "pCN"):                                   # the prior term applies to both updates
        assert {c[1] for c in SCORE_CASES if c[6] == kind} == {False, True}


def trivial_image(p, n):
    """The smallest emulator cesx_gp_set takes (the score kernels need one installed with n_gp = n_obs; they read none of it)."""
    return dict(n=n, Jt=1, p=p, A=np.tile(np.eye(p), (n, 1, 1)), c=np.zeros(p), Z=np.zeros((n, 1, p)),
                family=np.zeros(n, dtype=np.int32), par=np.tile([1.0, 0.1, 0.0], (n, 1)), mw=np.zeros((n, p)),
                alpha=np.zeros((n, 1)), Li=np.ones((n, 1, 1)))


def gp_case(eng_mod, mode, dense_sigma, p, n, M, dtype, kind, uniform=None, bad_var=False, part="C"):
    import torch
    ndt = np.dtype(dtype)
    rng = np.random.default_rng([GP_MODES.index(mode), int(dense_sigma), p, n, M, 1 if dtype == "float32" else 0,
                                 1 if kind else 0, int(bad_var)])
    like = "gamma" if mode == "gamma_dense" else mode
    gam = 0.1 + 0.1 * rng.random(n)
    Gamma = np.diag(gam)
    if mode == "gamma_dense":
        Bg = rng.standard_normal((n, n)) / np.sqrt(n)
        Gamma = 0.05 * (Bg @ Bg.T) + Gamma
    y = rng.standard_normal(n)
    mu = 0.1 * rng.standard_normal(p)
    if dense_sigma:
        Bs = rng.standard_normal((p, p)) / np.sqrt(p)
        Sigma = 0.5 * (Bs @ Bs.T) + 0.5 * np.eye(p)
    else:
        Sigma = np.diag(0.5 + rng.random(p))
    S = 0.3 * np.linalg.cholesky(Sigma)
    beta = 0.3
    kw, step_ids = {}, list(range(STEPS))
    if uniform is not None:
        seed, j_offset, step_ids = uniform
        kw = dict(seed=seed, j_offset=j_offset, J_global=j_offset + M)
    eng = eng_mod.Engine(p, n, M, dtype=dtype, **kw)
    eng.set_problem(y, Gamma, mu, Sigma, mu)
    eng.mh_set_proposal(kind, S, beta)
    eng.gp_set(trivial_image(p, n))
    want_var = like != "gamma"

    def rows():
        """synthetic GP rows: means a few noise standard deviations off the data, variances of the noise's size"""
        return y[:, None] + np.sqrt(gam)[:, None] * rng.standard_normal((n, M)), 0.05 + 0.1 * rng.random((n, M))

    def dev(a):
        return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=eng.device)

    def phi(Xh, mean, var):
        return sr.gp_phi(like, mean, var, y, Gamma, Xh.astype(np.float64), mu, Sigma)

    U_flat, U = guarded(eng, p)
    P_flat, P = guarded(eng, p)
    Uh = (mu[:, None] + 0.5 * rng.standard_normal((p, M))).astype(ndt)
    put(U, Uh)
    mean0, var0 = rows()
    keep = [dev(mean0), dev(var0)]
    eng.gp_start(like, U, keep[0], keep[1] if want_var else None)
    assert np.all(same_bits(U.cpu().numpy(), Uh)) and guards_intact(U_flat, U)
    ref = sr.AcceptRef(phi(Uh, mean0, var0))
    U0 = Uh.copy()
    # v <= 0 in chosen proposals: one negative, one exact zero, one zero where the mean meets the data (0 / 0)
    stuck = np.array([1, M // 2, M - 1]) if bad_var else np.zeros(0, dtype=int)

    def make_step(k, Uh):
        Ph = sr.propose(Uh.astype(np.float64), S, rng.standard_normal((p, M)), kind, beta).astype(ndt)
        mean, var = rows()
        logu = np.log(rng.random(M)) if uniform is None else sr.log_uniform(M, seed, step_ids[k], j_offset)
        if bad_var:
            off = gam if like == "gamma_var" else np.zeros(n)          # (gamma_var: v = Gamma_ii + var_i)
            i = k % n
            var[i, stuck[0]] = -off[i] - 0.3
            var[i, stuck[1]] = 0.0 - off[i]                            # (v = +0.0 exactly)
            var[i, stuck[2]] = 0.0 - off[i]
            mean[i, stuck[2]] = y[i]
            logu[stuck] = -1e6                                         # (any finite phi(P) would be accepted)
        return dict(P=Ph, mean=mean, var=var, phi_p=phi(Ph, mean, var), logu=logu)

    def launch(step, d):
        put(P, d["P"])
        keep[:] = [dev(d["mean"]), dev(d["var"])]
        lu = None if uniform is not None else dev(d["logu"])
        eng.gp_accept(like, step, U, P, keep[0], keep[1] if want_var else None, logu=lu)
        assert np.all(same_bits(P.cpu().numpy(), d["P"]))

    label = "gp_accept %s %s p=%d n=%d M=%d %s %s Sigma%s%s" % (
        dtype, mode, p, n, M, kind or "RW", "dense" if dense_sigma else "diagonal", " v<=0" if bad_var else "",
        " device uniform j_offset=%d" % uniform[1] if uniform else "")
    Uh, taken = run_accept_steps(eng, U_flat, U, Uh, ref, step_ids, make_step, launch, label, part)
    assert guards_intact(P_flat, P)
    if M >= 257:
        assert 0 < taken < len(step_ids) * M, (label, taken)
    if bad_var:
        assert np.all(ref.count[stuck] == 0) and np.all(same_bits(Uh[:, stuck], U0[:, stuck]))
    return ref


@pytest.mark.parametrize("mode,dense_sigma,p,n,M,dtype,kind", SCORE_CASES)
def test_score_against_fp64(eng_mod, mode, dense_sigma, p, n, M, dtype, kind):
    gp_case(eng_mod, mode, dense_sigma, p, n, M, dtype, kind)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("mode", ["var", "gamma_var"])
def test_a_non_positive_variance_rejects(eng_mod, mode, dtype):
    gp_case(eng_mod, mode, mode == "var", 8, 32, 257, dtype, None, bad_var=True)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("j_offset", [0, 2 ** 32 + 7])
@pytest.mark.parametrize("M", [5, 1023, 4099])
def test_score_with_the_device_uniform(eng_mod, M, j_offset, dtype):
    mode = GP_MODES[(M + (j_offset > 0)) % 4]
    gp_case(eng_mod, mode, M == 1023, 2, 4, M, dtype, "pCN" if M == 5 else None,
            uniform=(SEED, j_offset, UNIFORM_STEPS), part="B uniform (gp)")


# ---- D. gp_predict_kernel shapes -----------------------------------------------------------------------------------------

GP_T, GP_LDS_ROWS = 32, 608          # chains per tile; the panel stays in LDS up to J_p + p = 608 (kernels_gp.hip)
WORST = {"mean": 0.0, "var": 0.0}


def pad16(Jt):
    return (Jt + 15) // 16 * 16


def in_lds(Jt, p):
    return pad16(Jt) + p <= GP_LDS_ROWS


def pairs_and_slots(Jt, p, n, M):
    """(GP, tile) pairs and workgroup slots of the strided workspace path by the rule of the kernel's header: at most
    1024 slots and 256 MiB of panels of (J_p + p) x 32 doubles."""
    pairs = n * ((M + GP_T - 1) // GP_T)
    panel = (pad16(Jt) + p) * GP_T
    return pairs, max(1, min(pairs, 1024, (256 << 20) // (8 * panel)))


def np_predict_chunked(enka, X, nugget, chunk=1200):
    out = [np_predict(enka, enka.gpmodels, X[s:s + chunk], nugget) for s in range(0, len(X), chunk)]
    return (np.hstack([o[0] for o in out]), np.hstack([o[1] for o in out]), np.hstack([o[2] for o in out]), out[0][3])


def check_predict(enka, X, dtype="float64", label=""):
    """The device against np_predict with the bars of tests/test_gpu_gp.py, nugget on and off, mean-only = the mean."""
    m1, v1, Xh = device_predict(enka, X, True, dtype=dtype)
    m0, v0, _ = device_predict(enka, X, False, dtype=dtype)
    mo, vo, _ = device_predict(enka, X, True, var=False, dtype=dtype)
    mr, vr, sc, s2 = np_predict_chunked(enka, Xh, True)
    vr0 = np_predict_chunked(enka, Xh, False)[1]
    assert vo is None and np.array_equal(mo, m1) and np.array_equal(m0, m1)
    em_, ev1 = np.max(np.abs(m1 - mr) / (sc + 1e-300)), np.max(np.abs(v1 - vr) / s2[:, None])
    ev0 = np.max(np.abs(v0 - vr0) / s2[:, None])
    WORST["mean"], WORST["var"] = max(WORST["mean"], em_ / 1e-9), max(WORST["var"], ev1 / 1e-9, ev0 / 1e-9)
    print("gp_predict %s: mean err %.2e of sum |alpha k|, var err %.2e / %.2e of sigma^2 (bar 1e-9; worst ratios so far "
          "mean %.3g var %.3g)" % (label, em_, ev1, ev0, WORST["mean"], WORST["var"]))
    assert np.all(np.abs(m1 - mr) <= 1e-9 * (sc + 1e-300)), em_
    assert np.all(np.abs(v1 - vr) <= 1e-9 * s2[:, None]), ev1
    assert np.all(np.abs(v0 - vr0) <= 1e-9 * s2[:, None]), ev0
    return m1, v1, v0


def queries(rng, enka, M):
    """the first queries on training points (r = 0), the rest random"""
    Jt, p = enka.Ustar.shape[1], enka.p
    return np.vstack([enka.Ustar.T[:min(Jt, M)], rng.standard_normal((max(0, M - Jt), p))])[:M]


@pytest.fixture
def one_image(monkeypatch):
    """device_image once per emulator (np_predict and device_predict each rebuild it: a 2048^3 solve per GP and call)."""
    from ces_amd import emulate as em
    real, cache = em.device_image, {}

    def cached(enka, gps):
        key = (id(enka), tuple(id(g) for g in gps))
        if key not in cache:
            cache[key] = real(enka, gps)
        return cache[key]
    monkeypatch.setattr(em, "device_image", cached)


@pytest.mark.parametrize("M", [9600, 9593])
def test_predict_strides_over_the_workspace(one_image, M):
    """More (GP, tile) pairs than workgroup slots: every slot's zq, Kp and red are rewritten behind the trailing barrier."""
    Jt, p, n = 2048, 4, 2
    pairs, slots = pairs_and_slots(Jt, p, n, M)
    assert not in_lds(Jt, p) and pairs > slots, (pairs, slots)
    assert pairs_and_slots(Jt, p, n, 128)[0] <= pairs_and_slots(Jt, p, n, 128)[1]        # (128 queries: a single pass)
    rng = np.random.default_rng(M)
    enka = random_gps(rng, p, n, Jt, "Matern52", mean="Constant")
    X = queries(rng, enka, M)
    m1, v1, v0 = check_predict(enka, X, label="strided Jt=%d p=%d M=%d (%d pairs, %d slots)" % (Jt, p, M, pairs, slots))
    # the sum orders do not depend on the tile: the ends alone, in one pass, give the same bits
    ends = np.r_[0:64, M - 64:M]
    me, ve, _ = device_predict(enka, X[ends], True)
    _, ve0, _ = device_predict(enka, X[ends], False)
    assert np.array_equal(me, m1[:, ends]) and np.array_equal(ve, v1[:, ends]) and np.array_equal(ve0, v0[:, ends])


@pytest.mark.parametrize("Jt,p,lds", [(592, 16, True), (577, 16, True), (593, 15, False), (600, 8, False)])
def test_predict_at_the_lds_limit(one_image, Jt, p, lds):
    assert in_lds(Jt, p) == lds and (pad16(Jt) + p == GP_LDS_ROWS if lds else pad16(Jt) + p > GP_LDS_ROWS)
    rng = np.random.default_rng(Jt + p)
    enka = random_gps(rng, p, 2, Jt, "Matern32")
    check_predict(enka, queries(rng, enka, 70), label="LDS limit Jt=%d p=%d (%s)" % (Jt, p, "LDS" if lds else "workspace"))


@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("Jt", [77, 512])
@pytest.mark.parametrize("p", [8, 13, 20])
def test_predict_larger_input_dimensions(one_image, p, Jt, scaled):
    rng = np.random.default_rng(100 * p + Jt + int(scaled))
    enka = random_gps(rng, p, 3, Jt, FAMILIES[(p + Jt) % 4], scaled)
    check_predict(enka, queries(rng, enka, 100), dtype="float32" if scaled else "float64",
                  label="p=%d Jt=%d scaled=%d" % (p, Jt, scaled))


@pytest.mark.parametrize("scaled", [False, True])
def test_predict_32_gps_at_the_benchmarked_shape(one_image, scaled):
    rng = np.random.default_rng(32 + int(scaled))
    enka = random_gps(rng, 8, 32, 512, "Matern32", scaled)
    check_predict(enka, queries(rng, enka, 96), label="32 GPs p=8 Jt=512 scaled=%d" % scaled)


@pytest.mark.parametrize("k", [1, 7, 8, 9, 16, 17])
def test_predict_block_counts_around_the_zig_zag(one_image, k):
    rng = np.random.default_rng(k)
    enka = random_gps(rng, 3, 2, 16 * k, FAMILIES[k % 4])
    check_predict(enka, queries(rng, enka, 70), label="Jt=16*%d" % k)


@pytest.mark.parametrize("M", [1, 31, 32, 33])
def test_predict_query_counts_around_a_tile(one_image, M):
    rng = np.random.default_rng(M)
    enka = random_gps(rng, 3, 2, 77, "Matern52")
    check_predict(enka, queries(rng, enka, M), label="M=%d" % M)


def test_predict_mixed_families_and_means(one_image):
    """One image whose GPs differ in kernel family and mean function (par[4 g + 3] is per GP)."""
    rng = np.random.default_rng(12)
    p, Jt = 3, 77
    combos = list(itertools.product(FAMILIES, ["Zero", "Constant", "Linear"]))
    rng.shuffle(combos)
    n = len(combos)
    U = rng.standard_normal((p, Jt))
    G = np.vstack([np.sin(U[i % p]) + 0.1 * i for i in range(n)])
    enka = Enka(p, n, U, G)
    hyp = dict(ls=0.6 + 0.5 * rng.random((n, p)), var=0.5 + rng.random(n), lik=1e-4 * (1 + rng.random(n)),
               mA=0.3 * rng.standard_normal((n, p)), mb=rng.standard_normal(n))
    enka.gpmodels = [build_gps(U.T, G[i:i + 1], {k: v[i:i + 1] for k, v in hyp.items()}, fam, mean)[0]
                     for i, (fam, mean) in enumerate(combos)]
    assert {m.kern.family for m in enka.gpmodels} == {0, 1, 2, 3}
    assert [m.kern.family for m in enka.gpmodels] != sorted(m.kern.family for m in enka.gpmodels)
    check_predict(enka, queries(rng, enka, 203), label="mixed families and means")


# ---- E. kernels_gpfit.hip shapes -----------------------------------------------------------------------------------------

MEANS = ["Zero", "Constant", "Linear"]
FIT_WORST = {"lml": 0.0, "grad": 0.0}


def _fit_cases():
    cases = []
    # a second pass of the lengthscale sums (8 at a time): ARD at p = 9, 16, 17; p = 12 without ARD (one lengthscale)
    for k, ((p, ard), mean, Jt) in enumerate(itertools.product([(9, True), (16, True), (17, True), (12, False)], MEANS, [77, 300])):
        cases.append((k % 4, ard, mean, Jt, p))
    # block counts 1 .. 9 (the chunks of 4 of the block loops and the diagonal sum's stride of 8 with every remainder),
    # the 64 x 64 tile edges, and one J_t above 1024
    for k, Jt in enumerate([16 * b for b in range(1, 10)] + [63, 64, 65, 127, 129, 1030]):
        cases.append(((k + 1) % 4, k % 2 == 0, MEANS[k % 3], Jt, 3))
    return cases


FIT_CASES = _fit_cases()


def check_fit(rng, X, Y, fam, ard, mean, theta, label):
    """cesx_gpfit_eval against the host with the bar of tests/test_gpu_gpfit.py, and once more for the same bits."""
    from ces_amd import engine
    eng, nt = _engine(X, Y, fam, ard, mean)
    assert theta.shape[1] == nt
    lml, grad, status = eng.gpfit_eval(IDX, theta)
    assert np.all(status == engine.OK)
    for k, i in enumerate(IDX):
        hl, hg, dl, dg = _host_and_delta(rng, X, Y[i], fam, ard, mean, theta[k])
        assert np.isfinite(hl) and np.all(np.isfinite(hg))
        el, eg = abs(lml[k] - hl) / abs(hl), np.max(np.abs(grad[k] - hg)) / np.max(np.abs(hg))
        bl, bg = max(1e-9, 100 * dl), max(1e-9, 100 * dg)
        FIT_WORST["lml"], FIT_WORST["grad"] = max(FIT_WORST["lml"], el / bl), max(FIT_WORST["grad"], eg / bg)
        print("gpfit edges %s gp=%d: lml err %.2e (delta %.2e, ratio to bar %.3f) grad err %.2e (delta %.2e, ratio to bar "
              "%.3f); worst ratios so far lml %.3f grad %.3f"
              % (label, i, el, dl, el / bl, eg, dg, eg / bg, FIT_WORST["lml"], FIT_WORST["grad"]))
        assert el <= bl, (i, el, dl)
        assert eg <= bg, (i, eg, dg)
    eng.gpfit_eval(IDX[::-1], theta * 1.1)                           # (other values through the same workspace in between)
    again = eng.gpfit_eval(IDX, theta)
    assert np.array_equal(lml, again[0]) and np.array_equal(grad, again[1]) and np.array_equal(status, again[2])
    return eng


@pytest.mark.parametrize("fam,ard,mean,Jt,p", FIT_CASES)
def test_fit_shapes(fam, ard, mean, Jt, p):
    rng = np.random.default_rng(1000 * Jt + 10 * p + fam)
    X, Y = _problem(rng, Jt, p)
    check_fit(rng, X, Y, fam, ard, mean, _thetas(rng, len(IDX), p, ard, mean),
              "fam=%d ard=%d mean=%s Jt=%d p=%d" % (fam, ard, mean, Jt, p))


@pytest.mark.parametrize("ard", [True, False])
@pytest.mark.parametrize("fam", range(4))
def test_fit_on_coincident_training_inputs(fam, ard):
    """r = 0 off the diagonal (Matern-1/2 takes its g = 0 branch there).  sn^2 = 1e-2 keeps Ky positive definite: the
    host succeeds on the same input (check_fit asserts it), so the case is the kernel's and not a failed pivot."""
    Jt, p, mean = 77, 3, MEANS[fam % 3]
    rng = np.random.default_rng(500 + 2 * fam + int(ard))
    X, Y = _problem(rng, Jt, p)
    X[40] = X[3]
    X[11] = X[12] = X[10]
    check_fit(rng, X, Y, fam, ard, mean, _thetas(rng, len(IDX), p, ard, mean, sn2=1e-2),
              "coincident inputs fam=%d ard=%d mean=%s" % (fam, ard, mean))


def test_fit_factors_at_p16():
    """gpfit_factors against the host's factorisation with the bar of
    test_factors_of_a_device_fit_serve_device_image_and_predict: delta from K^{-1} = L^{-T} L^{-1} on permuted points."""
    fam, ard, mean, Jt, p = 2, True, "Linear", 77, 16
    rng = np.random.default_rng(16)
    X, Y = _problem(rng, Jt, p)
    theta = _thetas(rng, len(IDX), p, ard, mean)
    eng = check_fit(rng, X, Y, fam, ard, mean, theta, "factors p=16 Jt=77")
    for k, i in enumerate(IDX):
        alpha, Li = eng.gpfit_factors(i)
        m = _model(X, Y[i], fam, ard, mean, theta[k])
        L, al = m._factor()
        Lih = np.linalg.solve(L, np.eye(Jt))
        perm = rng.permutation(Jt)
        Lp = _model(X[perm], Y[i][perm], fam, ard, mean, theta[k])._factor()[0]
        Lpi = np.linalg.solve(Lp, np.eye(Jt))
        Kp = np.empty((Jt, Jt))
        Kp[np.ix_(perm, perm)] = Lpi.T @ Lpi
        Kinv = Lih.T @ Lih
        delta = np.max(np.abs(Kp - Kinv)) / np.max(np.abs(Kinv))
        bar = max(1e-9, 100 * delta)
        ea, sa = np.max(np.abs(alpha - al.ravel())), np.max(np.abs(al))
        eL, sL = np.max(np.abs(Li - Lih)), np.linalg.norm(Lih, 2)
        FIT_WORST["factors"] = max(FIT_WORST.get("factors", 0.0), ea / (bar * sa), eL / (bar * sL))
        print("gpfit edges factors gp=%d: alpha err %.2e of %.2e, L^-1 err %.2e of %.2e (delta %.2e, bar %.2e; worst ratio "
              "so far %.3f)" % (i, ea, sa, eL, sL, delta, bar, FIT_WORST["factors"]))
        assert ea <= bar * sa and eL <= bar * sL
        assert np.all(np.triu(Li, 1) == 0)
