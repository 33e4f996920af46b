"""Training the emulators on device: cesx_gpfit_eval against GPR.log_marginal_likelihood_and_grad, its status word and
bit-reproducibility, the factors a device fit leaves for device_image, and train_gps(device=True) end to end.

The bar of the pointwise comparisons is measured per GP, not assumed: the host's own rounding noise moves with the
conditioning of Ky, so the host is evaluated a second time with the training points permuted (mathematically the same
number) and delta = |host - host permuted| (lml: relative to |lml|; gradient: relative to its largest entry).  The device
must be within max(1e-9, 100 delta) of the host: 1e-9 is the bar tests/test_gpu_gp.py holds the fp64 GP path to; the factor
100 because delta is one draw and the device's summation order is a third order, not one of the two compared."""
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_emulate_host import Enka  # noqa: E402
from gp_cases import fit_problem  # noqa: E402

pytestmark = pytest.mark.gpu
FAMILIES = ["RBF", "Matern12", "Matern32", "Matern52"]
MEANS = ["Zero", "Constant", "Linear"]
JTS = [1, 16, 77, 300, 512, 700]
PS = [1, 3, 8]
N_GP, IDX = 7, [5, 0, 3, 6, 2]                   # 7 GPs in the problem, 5 of them evaluated, permuted


def _cases():
    cases = []
    for fam in range(4):                                            # every family at the benchmarked shape ...
        cases.append((fam, fam % 2 == 0, MEANS[(fam + 2) % 3], 512, 8))
    for fam in range(4):                                            # ... and at ragged J_t above 256 (the blocked path, padded)
        cases.append((fam, fam % 2 == 1, MEANS[fam % 3], 300, 3))
        cases.append((fam, fam % 2 == 0, MEANS[(fam + 1) % 3], 700, (8, 1, 3, 8)[fam]))
    k = 0
    for rep in range(2):                                            # every (J_t, p) twice, the other settings cycling
        for Jt, p in itertools.product(JTS, PS):
            if Jt >= 512 and (p == 8 or rep == 1):                  # (the large shapes are covered above; the host side is slow)
                continue
            cases.append(((k + rep) % 4, (k // 2 + rep) % 2 == 0, MEANS[(k + 2 * rep) % 3], Jt, p))
            k += 1
    return cases


CASES = _cases()


def test_the_cases_cover_what_they_must():
    assert 38 <= len(CASES) <= 48 and len(set(CASES)) == len(CASES)
    assert {c[0] for c in CASES} == {0, 1, 2, 3} and {c[1] for c in CASES} == {True, False}
    assert {c[2] for c in CASES} == set(MEANS) and {c[3] for c in CASES} == set(JTS) and {c[4] for c in CASES} == set(PS)
    assert {c[0] for c in CASES if c[3] == 512 and c[4] == 8} == {0, 1, 2, 3}
    assert {c[0] for c in CASES if c[3] > 256 and c[3] % 16} == {0, 1, 2, 3}


def _problem(rng, Jt, p, n=N_GP):
    return fit_problem(rng, Jt, p, n)


def _thetas(rng, n, p, ard, mean, sn2=None):
    nl = p if ard else 1
    cols = [0.5 + 1.5 * rng.random((n, 1)), (0.5 + 2.5 * rng.random((n, nl))) * np.sqrt(p),
            (10.0 ** rng.uniform(-6, -2, (n, 1)) if sn2 is None else np.full((n, 1), sn2))]
    if mean == "Constant":
        cols.append(rng.standard_normal((n, 1)))
    elif mean == "Linear":
        cols.append(0.3 * rng.standard_normal((n, p + 1)))
    return np.hstack(cols)


def _model(X, y, fam, ard, mean, theta):
    from ces_amd import emulate as em
    p = X.shape[1]
    mf = {"Zero": None, "Constant": em.Constant(), "Linear": em.Linear(np.ones((p, 1)))}[mean]
    m = em.GPR(X, y[:, None], getattr(em, FAMILIES[fam])(input_dim=p, ARD=ard), mean_function=mf)
    npos = 2 + (p if ard else 1)
    m._set(theta[:npos], theta[npos:])
    return m


def _engine(X, Y, fam, ard, mean, dtype="float64"):
    from ces_amd import engine
    eng = engine.Engine(X.shape[1], 1, 1, dtype=dtype)
    nt = eng.gpfit_set(X, Y, fam, ard, mean.lower())
    return eng, nt


def _host_and_delta(rng, X, y, fam, ard, mean, theta):
    """host (lml, grad) and the reference's own noise (delta_lml, delta_grad) from a permutation of the training points"""
    l0, g0 = _model(X, y, fam, ard, mean, theta).log_marginal_likelihood_and_grad()
    perm = rng.permutation(X.shape[0])
    l1, g1 = _model(X[perm], y[perm], fam, ard, mean, theta).log_marginal_likelihood_and_grad()
    return l0, g0, abs(l0 - l1) / abs(l0), np.max(np.abs(g0 - g1)) / np.max(np.abs(g0))


WORST = {"lml": 0.0, "grad": 0.0}


@pytest.mark.parametrize("fam,ard,mean,Jt,p", CASES)
def test_eval_matches_the_host_likelihood_and_gradient(fam, ard, mean, Jt, p):
    from ces_amd import engine
    rng = np.random.default_rng(1000 * Jt + 10 * p + fam)
    X, Y = _problem(rng, Jt, p)
    eng, nt = _engine(X, Y, fam, ard, mean, dtype="float32" if (Jt + p) % 2 else "float64")   # (fp64 whatever the engine dtype)
    theta = _thetas(rng, len(IDX), p, ard, mean)
    assert theta.shape[1] == nt
    lml, grad, status = eng.gpfit_eval(IDX, theta)
    assert np.all(status == engine.OK)
    for k, i in enumerate(IDX):
        hl, hg, dl, dg = _host_and_delta(rng, X, Y[i], fam, ard, mean, theta[k])
        el, eg = abs(lml[k] - hl) / abs(hl), np.max(np.abs(grad[k] - hg)) / np.max(np.abs(hg))
        bl, bg = max(1e-9, 100 * dl), max(1e-9, 100 * dg)
        WORST["lml"], WORST["grad"] = max(WORST["lml"], el / bl), max(WORST["grad"], eg / bg)
        print("gpfit parity fam=%d ard=%d mean=%s Jt=%d p=%d gp=%d: lml err %.2e (delta %.2e, ratio to bar %.3f) grad err %.2e "
              "(delta %.2e, ratio to bar %.3f); worst ratios so far lml %.3f grad %.3f"
              % (fam, ard, mean, Jt, p, i, el, dl, el / bl, eg, dg, eg / bg, WORST["lml"], WORST["grad"]))
        assert el <= bl, (i, el, dl)
        assert eg <= bg, (i, eg, dg)


@pytest.mark.parametrize("fam", range(4))
@pytest.mark.parametrize("Jt", [77, 300])
def test_a_failed_pivot_is_that_gps_alone(fam, Jt):
    from ces_amd import engine
    p, ard, mean = 3, True, "Linear"
    rng = np.random.default_rng(Jt + fam)
    X, Y = _problem(rng, Jt, p)
    eng, _ = _engine(X, Y, fam, ard, mean)
    theta = _thetas(rng, len(IDX), p, ard, mean, sn2=1e-3)
    theta[2, 1 + p] = -0.5                                           # Ky = K - I / 2 is indefinite
    with pytest.raises(np.linalg.LinAlgError):
        _model(X, Y[IDX[2]], fam, ard, mean, theta[2]).log_marginal_likelihood_and_grad()
    lml, grad, status = eng.gpfit_eval(IDX, theta)
    assert status[2] == engine.ENOTPD and np.all(np.delete(status, 2) == engine.OK)
    for k, i in enumerate(IDX):
        if k == 2:
            continue
        hl, hg, dl, dg = _host_and_delta(rng, X, Y[i], fam, ard, mean, theta[k])
        assert abs(lml[k] - hl) <= max(1e-9, 100 * dl) * abs(hl)
        assert np.max(np.abs(grad[k] - hg)) <= max(1e-9, 100 * dg) * np.max(np.abs(hg))
    # and the GP recovers at the next evaluation
    theta[2, 1 + p] = 1e-3
    lml2, grad2, status2 = eng.gpfit_eval(IDX, theta)
    assert np.all(status2 == engine.OK)
    hl, hg, dl, dg = _host_and_delta(rng, X, Y[IDX[2]], fam, ard, mean, theta[2])
    assert abs(lml2[2] - hl) <= max(1e-9, 100 * dl) * abs(hl)


@pytest.mark.parametrize("fam,ard,mean,Jt,p", [(2, True, "Linear", 512, 8), (0, False, "Constant", 77, 3), (3, True, "Zero", 300, 1)])
def test_two_evaluations_are_bit_identical(fam, ard, mean, Jt, p):
    rng = np.random.default_rng(Jt)
    X, Y = _problem(rng, Jt, p)
    eng, _ = _engine(X, Y, fam, ard, mean)
    theta = _thetas(rng, len(IDX), p, ard, mean)
    a = eng.gpfit_eval(IDX, theta)
    eng.gpfit_eval(IDX[::-1], theta * 1.1)                           # (other values through the same workspace in between)
    b = eng.gpfit_eval(IDX, theta)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def test_a_grid_larger_than_what_is_resident_at_once():
    """300 GPs at J_t = 300: every factorisation launch has 5 x 300 = 1500 workgroups, more than the card holds at once
    (5 waves per SIMD of gpfit_chol_kernel: 1280 workgroups of 4 waves on 256 CUs), so workgroups of a launch start after
    others of it have finished: nothing a launch reads may be written in it.  All 300 GPs are evaluated; 8 spread over
    the grid (the first and last included) are checked against the host, and the call is repeated bit for bit."""
    from ces_amd import engine
    fam, ard, mean, Jt, p, n = 2, True, "Linear", 300, 3, 300
    rng = np.random.default_rng(77)
    X, Y = _problem(rng, Jt, p, n)
    eng, _ = _engine(X, Y, fam, ard, mean)
    theta = _thetas(rng, n, p, ard, mean)
    idx = rng.permutation(n)
    a = eng.gpfit_eval(idx, theta)
    b = eng.gpfit_eval(idx, theta)
    assert np.all(a[2] == engine.OK) and np.all(np.isfinite(a[0])) and np.all(np.isfinite(a[1]))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    for k in (0, 1, 43, 127, 128, 255, 298, 299):
        hl, hg, dl, dg = _host_and_delta(rng, X, Y[idx[k]], fam, ard, mean, theta[k])
        el, eg = abs(a[0][k] - hl) / abs(hl), np.max(np.abs(a[1][k] - hg)) / np.max(np.abs(hg))
        print("gpfit large grid slot %d gp %d: lml err %.2e (delta %.2e) grad err %.2e (delta %.2e)" % (k, idx[k], el, dl, eg, dg))
        assert el <= max(1e-9, 100 * dl) and eg <= max(1e-9, 100 * dg), (k, el, dl, eg, dg)
    # every GP against a second engine that evaluates them eight at a time (grids far below residency)
    eng2, _ = _engine(X, Y, fam, ard, mean)
    for s in range(0, n, 8):
        l2, g2, s2 = eng2.gpfit_eval(idx[s:s + 8], theta[s:s + 8])
        assert np.array_equal(l2, a[0][s:s + 8]) and np.array_equal(g2, a[1][s:s + 8]), s


def test_bad_arguments():
    rng = np.random.default_rng(0)
    X, Y = _problem(rng, 20, 2)
    eng, nt = _engine(X, Y, 2, True, "Zero")
    th = _thetas(rng, 2, 2, True, "Zero")
    with pytest.raises(ValueError):
        eng.gpfit_eval([0, 0], th)                                   # a GP twice in one call
    with pytest.raises(ValueError):
        eng.gpfit_eval([0, N_GP], th)
    with pytest.raises(ValueError):
        eng.gpfit_set(X, Y, 7)
    with pytest.raises(Exception):
        eng.gpfit_eval([0, 1], th)                                   # the failed set left the handle without a fit problem


def _fit_problem(n=6):
    rng = np.random.default_rng(8)
    U = rng.standard_normal((2, 60))
    G = np.vstack([U[0] + 0.2 * U[1] ** 2, np.sin(U[1]), U.sum(0), np.cos(U[0]) * U[1], np.tanh(U[0] - U[1]),
                   0.5 * U[0] ** 2 - U[1]])[:n]
    return rng, U, G


def _host_lml(m):
    return m.log_marginal_likelihood_and_grad()[0]


def test_factors_of_a_device_fit_serve_device_image_and_predict():
    from ces_amd import emulate as em
    from test_gpu_gp import np_predict
    rng, U, G = _fit_problem(3)
    enka = Enka(2, 3, U, G)
    em.train_gps(enka, kernel="Matern32", mean_function="Linear", maxiter=300, device=True)
    img = em.device_image(enka, enka.gpmodels)
    for i, m in enumerate(enka.gpmodels):
        assert np.array_equal(img["alpha"][i], m._device_factors[1]) and np.array_equal(img["Li"][i], m._device_factors[2])
        L, al = m._factor()
        Li = np.linalg.solve(L, np.eye(60))
        perm = rng.permutation(60)
        mp = em.GPR(m.X[perm], m.Y[perm], m.kern, mean_function=m.mean_function)
        mp.likelihood.variance = m.likelihood.variance
        # the reference's own noise in this factorisation: K^{-1} = L^{-T} L^{-1} from the permuted points, permuted back
        # (alpha would do as well, but it is exactly 0 for an output the Linear mean fits exactly)
        Lp = mp._factor()[0]
        Lpi = np.linalg.solve(Lp, np.eye(60))
        Kp = np.empty((60, 60))
        Kp[np.ix_(perm, perm)] = Lpi.T @ Lpi
        Kinv = Li.T @ Li
        delta = np.max(np.abs(Kp - Kinv)) / np.max(np.abs(Kinv))
        bar = max(1e-9, 100 * delta)
        ea, sa = np.max(np.abs(img["alpha"][i] - al.ravel())), np.max(np.abs(al))
        eL, sL = np.max(np.abs(img["Li"][i] - Li)), np.linalg.norm(Li, 2)
        print("gpfit factors gp=%d: alpha err %.2e of %.2e, L^-1 err %.2e of %.2e (delta %.2e, bar %.2e)" % (i, ea, sa, eL, sL, delta, bar))
        assert ea <= bar * sa and eL <= bar * sL
        assert np.all(np.triu(img["Li"][i], 1) == 0)
    X = np.vstack([U.T[:10], rng.standard_normal((90, 2))])
    for nugget in (True, False):
        hm, hv = em.predict_gps(enka, X, nugget=nugget)
        dm, dv = em.predict_gps(enka, X, nugget=nugget, device=True)
        mr, vr, sc, s2 = np_predict(enka, enka.gpmodels, X, nugget)
        assert np.all(np.abs(dm - hm) <= 1e-9 * sc)
        assert np.all(np.abs(dv - hv) <= 1e-9 * s2[:, None] + 1e-9 * np.abs(hv))
    # other training data under the same parameters: the host factorisation again, silently
    m = enka.gpmodels[1]
    keepY = m.Y
    m.Y = m.Y + 0.01
    img3 = em.device_image(enka, enka.gpmodels)
    assert not np.array_equal(img3["alpha"][1], img["alpha"][1])
    assert np.allclose(img3["alpha"][1], m._factor()[1].ravel(), rtol=0, atol=1e-12 * np.max(np.abs(img3["alpha"][1])))
    m.Y = keepY
    # changed parameters: the host factorisation again, silently
    m = enka.gpmodels[0]
    m.likelihood.variance *= 2.0
    img2 = em.device_image(enka, enka.gpmodels)
    assert np.allclose(img2["alpha"][0], m._factor()[1].ravel(), rtol=0, atol=1e-12 * np.max(np.abs(img2["alpha"][0])))
    assert not np.array_equal(img2["alpha"][0], img["alpha"][0])


def test_train_gps_device_end_to_end():
    """Fitted parameters cannot be compared tightly (the likelihood is flat along some directions and L-BFGS-B's stop is
    loose), so: every fit succeeds, raises the host-evaluated lml above its start, and ends within 10 x the reference's
    own spread (host fit against host fit on permuted points, the largest over the GPs) of the host fit's lml.
    (Measured: spreads of the reference 5.7e-14 .. 5.6e-1, of the device fit against the host fit 0 .. 3.1e-1.  The
    ``success`` flag is L-BFGS-B's line search not giving up at the noise floor of an ill-conditioned Ky; a host fit on
    permuted points can lose it too -- NOTEBOOK.md, "Emulate: training on device".)"""
    from ces_amd import emulate as em
    rng, U, G = _fit_problem(6)
    n = 6
    kw = dict(kernel="Matern32", mean_function="Linear", maxiter=300)
    start = [_host_lml(em.GPR(U.T, G[i][:, None], em.Matern32(input_dim=2, ARD=True), mean_function=em.Linear(np.ones((2, 1)))))
             for i in range(n)]
    host = Enka(2, n, U, G)
    em.train_gps(host, **kw)
    perm = rng.permutation(60)
    hostp = Enka(2, n, U[:, perm], G[:, perm])
    em.train_gps(hostp, **kw)
    dev = Enka(2, n, U, G)
    em.train_gps(dev, device=True, **kw)
    lh = np.array([_host_lml(m) for m in host.gpmodels])
    lp = np.array([_host_lml(m) for m in hostp.gpmodels])
    ld = np.array([_host_lml(m) for m in dev.gpmodels])
    spread_ref, spread_dev = np.abs(lh - lp), np.abs(ld - lh)
    print("gpfit end to end: host lml %s\n  |host - host permuted| %s\n  |device fit - host fit| %s" % (lh, spread_ref, spread_dev))
    assert len(dev.gpmodels) == n
    for i, m in enumerate(dev.gpmodels):
        assert isinstance(m, em.GPR) and m.optimizer.result.success, i
        assert ld[i] > start[i], i
    assert np.all(spread_dev <= 10 * spread_ref.max()), (spread_dev, spread_ref)


def test_train_gps_device_twice_gives_identical_parameters():
    from ces_amd import emulate as em
    _, U, G = _fit_problem(4)
    fits = []
    for _ in range(2):
        enka = Enka(2, 4, U, G)
        em.train_gps(enka, kernel="Matern52", mean_function="Constant", maxiter=100, device=True)
        fits.append(np.array([np.concatenate(m._get()) for m in enka.gpmodels]))
    assert np.array_equal(fits[0], fits[1])
