"""The Lorenz '63 forward map on the device (cesx_lorenz_three_*, ces_amd/csrc/kernels_l63.hip: one particle per lane) against
scipy's RK45 on the host model, within an envelope computed from the host alone (tests/l63_cases.py), and the device-resident
pde run built on it."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import l63_cases as lc  # noqa: E402

pytestmark = pytest.mark.gpu


def _engine(J, dtype="float64", n_obs=9):
    from ces_amd import engine
    return engine.Engine(2, n_obs, J, dtype=dtype)


def _apply(model, eng, U, W0, t, **kw):
    """(G, W, info) on the host for host inputs U (2, J), W0 (3, J)."""
    import torch
    model.ensure_installed(eng, t)
    Ud = eng.to_device(np.ascontiguousarray(U), 2, "U")
    Wd = torch.as_tensor(np.array(W0, order="C"), device=eng.device)           # (a copy: the references are read-only)
    G, W, info = eng.l63_apply(Ud, Wd, **kw)
    return G.cpu().numpy().astype(np.float64), W.cpu().numpy(), info.cpu().numpy()


CASES = ([(name, 1, J, dtype) for name in lc.CLASSES for J in (1, 63, 64, 65, 257) for dtype in ("float64", "float32")]
         + [("lorenz63", 2, 65, "float64"), ("lorenz63_log", 2, 65, "float32"), ("lorenz63_log", 4, 48, "float64")])


@pytest.mark.parametrize("name, T, J, dtype", CASES, ids=["%s-T%g-J%d-%s" % c for c in CASES])
def test_against_solve_ivp(name, T, J, dtype):
    """End state, statistics, step counts and status 0 of every particle against the host's ``solve_ivp`` run: a partial wave,
    a full wave, one lane over and a ragged last wave of several, both engine dtypes, both classes."""
    ref = lc.reference(name, T, dtype)
    cols = lc.columns(J)
    m = lc.make_model(name)
    G, W, info = _apply(m, _engine(J, dtype), ref["U"][:, cols], ref["W0"][:, cols], ref["t"])
    assert np.all(info[3] == 0)
    lc.check_against(ref, dtype, G, W, info)


def test_a_wave_of_lanes_that_disagree():
    """Adjacent lanes alternate r = 0.5 (the origin attracts: long steps) and r = 28 (chaotic: short steps), from two starts
    each: every lane's outputs and step counts are bitwise those of its own single-particle run."""
    m = lc.make_model("lorenz63")
    t = lc.times(4.0)
    S = lc.attractor_states()
    kinds = [(0.5, 0), (28.0, 1), (0.5, 2), (28.0, 3)]
    J = 66
    U = np.array([[kinds[j % 4][0] for j in range(J)], [8.0 / 3] * J])
    W0 = np.stack([S[:, kinds[j % 4][1]] for j in range(J)], axis=1)
    big = _apply(m, _engine(J), U, W0, t)
    assert np.all(big[2][0] == 0)
    for k in range(4):
        one = _apply(m, _engine(1), U[:, [k]], W0[:, [k]], t)
        for j in range(k, J, 4):
            for a, b in zip(big, one):
                assert np.array_equal(a[:, j], b[:, 0]), (k, j)
    att = big[2][2]
    print("attempted steps, r = 0.5 / 28:", att[0], att[2], "/", att[1], att[3])
    assert max(att[0], att[2]) < min(att[1], att[3])          # the lanes of the wave did run different step sequences


def test_reproducible_and_placement_free():
    """Two calls are bitwise equal; a particle's three outputs are bitwise the same alone, as column 0, as column 64 and as the
    last column of J = 257 -- also with ``out=`` / ``W_out=`` given and with ``W_out`` aliasing ``W``."""
    import torch
    m = lc.make_model("lorenz63_log")
    t = lc.times(2.0)
    U, S = lc.class_params("lorenz63_log")
    J = 257
    cols = np.arange(J) % 5
    cols[[0, 64, 256]] = 7
    eng = _engine(J)
    big = _apply(m, eng, U[:, cols], S[:, cols], t)
    again = _apply(m, eng, U[:, cols], S[:, cols], t)
    for a, b in zip(big, again):
        assert np.array_equal(a, b)
    assert np.all(big[2][0] == 0)
    one = _apply(m, _engine(1), U[:, [7]], S[:, [7]], t)
    for c in (0, 64, 256):
        for a, b in zip(big, one):
            assert np.array_equal(a[:, c], b[:, 0]), c
    first = {k: int(np.flatnonzero(cols == k)[0]) for k in set(cols)}      # the first column that holds particle k
    for c in range(J):                                         # every copy of a particle, wherever it sits
        for a in big:
            assert np.array_equal(a[:, c], a[:, first[cols[c]]]), c
    # given outputs, and W_out aliasing W
    m.ensure_installed(eng, t)
    Ud = eng.to_device(np.ascontiguousarray(U[:, cols]), 2, "U")
    Wd = torch.as_tensor(np.array(S[:, cols], order="C"), device=eng.device)
    out, W_out = eng.empty(9), torch.empty_like(Wd)
    G, W, info = eng.l63_apply(Ud, Wd, out=out, W_out=W_out)
    assert G is out and W is W_out
    assert np.array_equal(G.cpu().numpy(), big[0]) and np.array_equal(W.cpu().numpy(), big[1])
    G2, W2, info2 = eng.l63_apply(Ud, Wd, W_out=Wd)
    assert W2 is Wd
    assert np.array_equal(G2.cpu().numpy(), big[0]) and np.array_equal(Wd.cpu().numpy(), big[1])
    assert np.array_equal(info2.cpu().numpy(), big[2])


def test_failures_are_reported_not_spun():
    """Every failing particle ends in a status code and the kernel returns normally; its outputs are NaN and its neighbours
    agree with the host as in test_against_solve_ivp.  r = 1e308: the tendencies overflow in the first attempt, status 2.
    ``max_attempts = 5``: status 3 for every particle.  Then: CESX_EINVAL keeps the installed map."""
    import torch
    from ces_amd import engine
    name, T, J = "lorenz63", 1, 8
    ref = lc.reference(name, T, "float64")
    t = ref["t"]
    m = lc.make_model(name)
    eng = _engine(J)
    U, W0 = np.array(ref["U"][:, :J]), ref["W0"][:, :J]
    U[0, 2] = 1e308
    G, W, info = _apply(m, eng, U, W0, t)
    assert list(info[0]) == [0, 0, 2, 0, 0, 0, 0, 0]
    assert np.all(np.isnan(G[:, 2])) and np.all(np.isnan(W[:, 2]))
    keep = np.array([0, 1, 3, 4, 5, 6, 7])
    lc.check_against(ref, "float64", G[:, keep], W[:, keep], info[:, keep], cols=keep)
    Wd = torch.as_tensor(np.array(W0, order="C"), device=eng.device)
    with pytest.raises(ValueError, match="particle 2 failed with status 2"):
        m.forward_pde_device(eng, eng.to_device(U, 2, "U"), Wd, t)
    Gd, _ = m.forward_pde_device(eng, eng.to_device(U, 2, "U"), Wd, t, check=False)        # no read-back, no exception
    assert np.array_equal(np.isnan(Gd.cpu().numpy()).any(axis=0), info[0] != 0)

    m.device_max_attempts = 5
    G, W, info = _apply(m, eng, ref["U"][:, :J], W0, t)
    assert np.all(info[0] == 3) and np.all(info[2] == 5) and np.all(info[1] <= 5)
    assert np.all(np.isnan(G)) and np.all(np.isnan(W))
    m.device_max_attempts = 1000000
    assert engine.L63_STATUS[3].startswith("max_attempts")

    # CESX_EINVAL keeps the installed map
    G0, W_0, info0 = _apply(m, eng, ref["U"][:, :J], W0, t)
    d = m.device_descriptor(t, 2, 9)
    for bad in (dict(par_row=np.array([-1, 0, 2])), dict(par_row=np.array([-1, 0, 0])), dict(par_row=np.array([-2, 0, 1])),
                dict(par_fixed=np.array([np.nan, 0.0, 0.0])), dict(t=t[::-1].copy()), dict(t=t * 2), dict(t=t - 0.5),
                dict(window_samples=3), dict(window_samples=0), dict(rtol=0.0), dict(atol=-1.0), dict(max_step=0.0),
                dict(T=0.0), dict(t0=np.inf), dict(max_attempts=0), dict(t=t[:1])):
        with pytest.raises(ValueError, match="cesx_lorenz_three_set"):     # (Engine._check maps CESX_EINVAL to ValueError)
            eng.l63_set(dict(d, **bad))
    with pytest.raises(ValueError, match="n_obs is not 9"):
        _engine(J, n_obs=8).l63_set(d)
    Ud = eng.to_device(np.ascontiguousarray(ref["U"][:, :J]), 2, "U")
    G1, W1, info1 = eng.l63_apply(Ud, Wd)                   # no install in between: the map of before the bad descriptors
    assert np.array_equal(G1.cpu().numpy(), G0) and np.array_equal(W1.cpu().numpy(), W_0)
    lc.check_against(ref, "float64", G0, W_0, info0)


def test_device_resident_pde_run():
    """``sampling.run`` on a ``lorenz63`` model with the hook against the plain host loop (``solve`` after ``set_solver``) on
    the same injected noise.  Iteration 0 is compared within the envelope (``Gall[0]``) and within that envelope pushed through
    the update (``Uall[1]``), as tests/test_gpu_l96.py::test_device_resident_pde_run does; from then on the trajectories differ
    by more than rounding and only shapes, finiteness and the bookkeeping are checked.  A ``ws=`` run keeps the plain loop."""
    from ces_amd.calibrate import sampling
    name, T, J, iters = "lorenz63", 2, 64, 3
    ref = lc.reference(name, T, "float64")
    cols = lc.columns(J)
    t = ref["t"]
    rs = np.random.RandomState(3)
    y_obs = ref["G"].mean(axis=1) * (1.0 + 0.02 * rs.standard_normal(9))
    Gamma = np.diag((0.05 * np.abs(ref["G"]).mean(axis=1) + 0.1) ** 2)
    xis = rs.standard_normal((iters, 2, J))
    wt = np.array(lc.attractor_states()[:, 5])
    U0 = np.array(ref["U"][:, cols])

    def run(device, **kw):
        m = lc.make_model(name, device=device)
        calls = []
        if device:
            hook = m.forward_pde_device
            m.forward_pde_device = lambda *a, **k: (calls.append(1), hook(*a, **k))[1]
        eks = sampling(p=2, n_obs=9, J=J)
        eks.T = iters
        eks.mu, eks.sigma, eks.ustar = np.array([28.0, 8.0 / 3]), np.diag([25.0, 0.25]), np.array([28.0, 8.0 / 3])
        eks.run(y_obs, U0.copy(), m, Gamma, None, wt=wt, t=t, xis=xis, t_tol=1e9, **kw)
        return eks, calls

    host, _ = run(False)
    dev, calls = run(True)
    assert len(calls) == iters + 1
    for eks in (host, dev):
        assert eks.Uall.shape == (iters + 1, 2, J) and eks.Gall.shape == (iters + 1, 9 + 3, J)
        assert np.all(np.isfinite(eks.Uall)) and np.all(np.isfinite(eks.Gall))
        assert isinstance(eks.W0, np.ndarray) and eks.W0.shape == (3, J) and eks.W0.dtype == np.float64
        assert np.array_equal(eks.W0, eks.Gall[-1][9:]) and np.array_equal(eks.Gstar, eks.Gall[-1][:9])
        assert np.array_equal(eks.Ustar, eks.Uall[-1]) and len(eks.metrics["t"]) == iters
        assert not hasattr(eks, "Wall")
    # iteration 0: every particle starts from wt; the envelope of that evaluation, from the host alone
    m = lc.make_model(name, device=False)
    env = 0.0
    for j in range(0, J, 8):
        clean = lc.host_run(m, wt, t, tuple(U0[:, j]))
        for seed in (1, 2, 3, 4):
            r = lc.host_run(m, wt, t, tuple(U0[:, j]), noise_seed=seed)
            env = max(env, np.abs(np.r_[r["stats"], r["end"]] - np.r_[clean["stats"], clean["end"]]).max()
                      / np.abs(np.r_[clean["stats"], clean["end"]]).max())
    assert env <= lc.ENV_MAX
    scale = np.abs(host.Gall[0]).max()
    tol = (4 * env + (64 + lc.WINDOW) * lc.EPS) * scale
    dG = np.abs(dev.Gall[0] - host.Gall[0]).max()
    dU = np.abs(dev.Uall[1] - host.Uall[1]).max()
    print("pde run: env %.2e dG %.2e tol %.2e dU %.2e" % (env, dG, tol, dU))
    assert np.array_equal(dev.Uall[0], host.Uall[0])
    assert dG <= tol
    assert dU <= 1e3 * tol * max(1.0, np.abs(host.Uall[1]).max() / scale)

    lib, calls = run(True, ws=np.tile(wt, (4, 1)))
    assert not calls and len(lib.Wall) == iters + 1                  # the library draw keeps the plain loop


def test_long_window_in_distribution():
    """The notebook's window against the reference's integrator: 64 starts on the attractor, r = 28, b = 8/3, l_window = 10,
    freq = 100, t = linspace(0, 20, 2001); per statistic the device's (RK45) ensemble mean against the host's ``odeint`` mean
    within 5 standard errors of the difference.  The starts are NOT the first 64 of the pointwise cases' table: those lie 0.37
    time units apart on one trajectory, so their windows overlap and are no independent samples (host RK45 against ``odeint``
    reaches 4.2 standard errors there); these lie one window length apart (``l63_cases.independent_starts``), for which host
    RK45 against ``odeint`` on the CPU gives at most 1.11 and the kernel at most 1.46.  Fixed inputs: the verdict is
    deterministic."""
    from ces_amd import models
    J = 64
    t = np.linspace(0.0, 20.0, 2001)
    starts = lc.independent_starts(J)               # a window length apart: the 64 windows are independent samples
    host = models.lorenz63(l_window=10, freq=100)                     # no set_solver: odeint, as the reference integrates
    Gh = np.stack([host.statistics(host.solve(starts[:, j], t, args=(28.0, 8.0 / 3))) for j in range(J)], axis=1)
    m = lc.make_model("lorenz63", l_window=10, freq=100)
    U = np.tile(np.array([[28.0], [8.0 / 3]]), (1, J))
    G, W, info = _apply(m, _engine(J), U, starts, t)
    assert np.all(info[0] == 0) and np.all(np.isfinite(G)) and np.all(np.isfinite(W))
    se = np.sqrt(Gh.var(axis=1, ddof=1) / J + G.var(axis=1, ddof=1) / J)
    z = np.abs(G.mean(axis=1) - Gh.mean(axis=1)) / se
    print("long window: |dmean| / se =", np.round(z, 3))
    assert np.all(z <= 5.0)
