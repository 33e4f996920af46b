"""The Lorenz '96 forward map on the device (cesx_lorenz_*, ces_amd/csrc/kernels_l96.hip) against scipy's RK45 on the host
model, within an envelope computed from the host alone (tests/l96_cases.py), and the device-resident pde run built on it."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import l96_cases as lc  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "l96_long.npz")


def _engine(p, n_obs, J, dtype):
    from ces_amd import engine
    return engine.Engine(p, n_obs, J, dtype=dtype)


def _apply(model, eng, U, W0, t, **kw):
    """(G, W, info) on the host for host inputs U (p, J), W0 (n_state, J)."""
    import torch
    model.ensure_installed(eng, t)
    Ud = eng.to_device(np.ascontiguousarray(U), U.shape[0], "U")
    Wd = torch.as_tensor(np.ascontiguousarray(W0), device=eng.device)
    G, W, info = eng.l96_apply(Ud, Wd, **kw)
    return G.cpu().numpy().astype(np.float64), W.cpu().numpy(), info.cpu().numpy()


CASES = ([("lorenz96", shape, 0.2, J, dtype, None)
          for shape in ((4, 1), (5, 3), (36, 10)) for J in (1, 65, 96) for dtype in ("float64", "float32")]
         + [("lorenz96", (36, 10), 0.5, 16, dtype, None) for dtype in ("float64", "float32")]
         + [(name, (5, 3), 0.2, 8, "float64", None) for name in lc.CLASSES[1:]]
         + [("lorenz96", (5, 3), 0.2, 8, "float64", 0.15)])


@pytest.mark.parametrize("name, shape, T, J, dtype, t_last", CASES,
                         ids=["%s-%dx%d-T%g-J%d-%s%s" % (c[0], c[1][0], c[1][1], c[2], c[3], c[4], "-short" if c[5] else "")
                              for c in CASES])
def test_against_solve_ivp(name, shape, T, J, dtype, t_last):
    """End state, statistics, step counts and status 0 of every particle against the host's ``solve_ivp`` run.  One stripe of
    lanes (n_state 8), a ragged stripe (20), seven stripes with a ragged last one (396); every class's parameter map; once
    with t[-1] < T, where the device stops after the last sample and only the outputs are compared."""
    Jref = 96 if J in (1, 65, 96) and T == 0.2 and name == "lorenz96" else J       # one reference for the three ensemble sizes
    ref = lc.reference(name, shape, T, dtype, Jref, t_last)
    m = lc.make_model(name, shape, T=T)
    eng = _engine(ref["U"].shape[0], ref["G"].shape[0], J, dtype)
    G, W, info = _apply(m, eng, ref["U"][:, :J], ref["W0"][:, :J], ref["t"])
    assert np.all(info[3] == 0)
    lc.check_against(ref, dtype, G, W, info, counts=t_last is None)


def test_reproducible_and_placement_free():
    """Two calls are bitwise equal; a particle's three outputs are bitwise the same alone, as column 0, as column 64 and as the
    last column of J = 257 -- also with ``out=`` / ``W_out=`` given and with ``W_out`` aliasing ``W``."""
    import torch
    name, shape, T = "lorenz96", (36, 10), 0.2
    m = lc.make_model(name, shape, T=T)
    t = lc.times(T)
    U, S = lc.class_params(name, shape)
    J = 257
    cols = np.arange(J) % 5                                   # five distinct particles, repeated: column j holds particle j % 5
    cols[[0, 64, 256]] = 3
    eng = _engine(4, 180, J, "float64")
    big = _apply(m, eng, U[:, cols], S[:, cols], t)
    again = _apply(m, eng, U[:, cols], S[:, cols], t)
    for a, b in zip(big, again):
        assert np.array_equal(a, b)
    assert np.all(big[2][0] == 0)
    one = _apply(m, _engine(4, 180, 1, "float64"), U[:, [3]], S[:, [3]], t)
    for c in (0, 64, 256):
        for a, b in zip(big, one):
            assert np.array_equal(a[:, c], b[:, 0]), c
    first = {k: int(np.flatnonzero(cols == k)[0]) for k in range(5)}     # the first column that holds particle k
    for c in range(J):                                        # every copy of a particle, wherever it sits
        for a in big:
            assert np.array_equal(a[:, c], a[:, first[cols[c]]]), c
    # given outputs, and W_out aliasing W
    m.ensure_installed(eng, t)
    Ud = eng.to_device(np.ascontiguousarray(U[:, cols]), 4, "U")
    Wd = torch.as_tensor(np.ascontiguousarray(S[:, cols]), device=eng.device)
    out, W_out = eng.empty(180), torch.empty_like(Wd)
    G, W, info = eng.l96_apply(Ud, Wd, out=out, W_out=W_out)
    assert G is out and W is W_out
    assert np.array_equal(G.cpu().numpy(), big[0]) and np.array_equal(W.cpu().numpy(), big[1])
    G2, W2, info2 = eng.l96_apply(Ud, Wd, W_out=Wd)
    assert W2 is Wd
    assert np.array_equal(G2.cpu().numpy(), big[0]) and np.array_equal(Wd.cpu().numpy(), big[1])
    assert np.array_equal(info2.cpu().numpy(), big[2])


def test_failures_are_reported_not_spun():
    """Every failing particle ends in a status code and the kernel returns normally; its outputs are NaN and its neighbours
    agree with the host as in test_against_solve_ivp.

    * F = 1e308: the tendencies overflow in the first attempt, status 2 (scipy shrinks the step on the NaN error norm until it
      reports its step-size failure).
    * ``max_attempts = 5``: status 3 for every particle.
    * status 1 needs a step below ``10 * spacing(t)`` with every number finite.  The issue's b = 1e15 does not get there:
      scipy crawls at h ~ 1e-16 without ever failing (3000 steps reach t = 2.6e-13, checked on the CPU), as do b = 1e30 ..
      1e300.  What does fail in scipy with finite numbers is a ``max_step`` below the spacing at t > 0: dt = 1e-323 takes one
      step of min_step = 4.9e-323 from t = 0 and then finds max_step < min_step.  The test first asserts that scipy reports
      exactly that, then asks the device for status 1 after one accepted step."""
    import warnings
    from scipy.integrate import RK45
    from ces_amd import engine
    name, shape, T, J = "lorenz96", (5, 3), 0.2, 8
    ref = lc.reference(name, shape, T, "float64", J)
    t = ref["t"]
    m = lc.make_model(name, shape, T=T)
    eng = _engine(4, 25, J, "float64")
    U = np.array(ref["U"])
    U[1, 2] = 1e308
    G, W, info = _apply(m, eng, U, ref["W0"], t)
    assert list(info[0]) == [0, 0, 2, 0, 0, 0, 0, 0]
    assert np.all(np.isnan(G[:, 2])) and np.all(np.isnan(W[:, 2]))
    keep = np.array([0, 1, 3, 4, 5, 6, 7])
    lc.check_against(ref, "float64", G[:, keep], W[:, keep], info[:, keep], cols=keep)
    with pytest.raises(ValueError, match="particle 2 failed with status 2"):
        import torch
        m.forward_pde_device(eng, eng.to_device(U, 4, "U"), torch.as_tensor(np.ascontiguousarray(ref["W0"]), device=eng.device), t)

    m.device_max_attempts = 5
    G, W, info = _apply(m, eng, ref["U"], ref["W0"], t)
    assert np.all(info[0] == 3) and np.all(info[2] == 5) and np.all(info[1] <= 5)
    assert np.all(np.isnan(G)) and np.all(np.isnan(W))
    m.device_max_attempts = 1000000

    tiny = 1e-323
    host = lc.make_model(name, shape, T=T, dt=tiny, device=False)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        solver = RK45(lambda tt, y: host(tt, y, *ref["U"][:, 0]), 0.0, np.array(ref["W0"][:, 0]), T, max_step=tiny)
        messages = [solver.step(), solver.step()]
    assert solver.status == "failed" and messages[1] == solver.TOO_SMALL_STEP and np.all(np.isfinite(solver.y))
    m.set_solver(T=T, dt=tiny, device=True)
    G, W, info = _apply(m, eng, ref["U"], ref["W0"], t)
    assert np.all(info[0] == 1) and np.all(info[1] == 1) and np.all(info[2] == 1)
    assert np.all(np.isnan(G)) and np.all(np.isnan(W))
    assert engine.L96_STATUS[1].startswith("the step size fell below")

    # CESX_EINVAL keeps the installed map
    d = m.device_descriptor(t, 4, 25)
    for bad in (dict(n_slow=3, n_obs=15), dict(n_fast=0), dict(n_slow=50, n_fast=10), dict(p=3), dict(n_obs=24),
                dict(par_row=np.array([0, 1, 2, 4])), dict(par_row=np.array([0, 1, 1, 3])), dict(t=t[::-1].copy()),
                dict(t=t * 2), dict(spinup_samples=1), dict(window_samples=3), dict(rtol=0.0), dict(atol=-1.0), dict(T=0.0),
                dict(max_step=0.0)):
        with pytest.raises(ValueError, match="cesx_lorenz_set"):           # (Engine._check maps CESX_EINVAL to ValueError)
            eng.l96_set(dict(d, **bad))
    m.set_solver(T=T, dt=0.1, device=True)
    G, W, info = _apply(m, eng, ref["U"], ref["W0"], t)
    lc.check_against(ref, "float64", G, W, info)


def test_device_resident_pde_run():
    """``sampling.run`` on a ``lorenz96Fb`` model at (5, 3) with the hook against the plain host loop on the same injected
    noise.  Iteration 0 is compared within the envelope (``Gall[0]``) and within that envelope pushed through the update
    (``Uall[1]``); from then on the two trajectories differ by more than rounding (the ensemble update amplifies the
    difference, the next forward evaluation is chaotic) and only shapes, finiteness and the bookkeeping are checked."""
    from ces_amd.calibrate import sampling
    name, shape, T, J, iters = "lorenz96Fb", (5, 3), 0.2, 64, 3
    ref = lc.reference(name, shape, T, "float64", J)
    t = ref["t"]
    ns = 20
    rs = np.random.RandomState(3)
    y_obs = ref["G"].mean(axis=1) + 0.1 * rs.standard_normal(25)
    Gamma = np.diag(np.full(25, 0.5 ** 2))
    xis = rs.standard_normal((iters, 2, J))
    wt = np.array(lc.attractor_state(*shape))

    def run(device, **kw):
        m = lc.make_model(name, shape, T=T, device=device)
        calls = []
        if device:
            hook = m.forward_pde_device
            m.forward_pde_device = lambda *a, **k: (calls.append(1), hook(*a, **k))[1]
        eks = sampling(p=2, n_obs=25, J=J)
        eks.T = iters
        eks.mu, eks.sigma, eks.ustar = np.array([10.0, 10.0]), np.diag([9.0, 9.0]), np.array([10.0, 10.0])
        eks.run(y_obs, np.array(ref["U"]), m, Gamma, None, wt=wt, t=t, xis=xis, t_tol=1e9, **kw)
        return eks, calls

    host, _ = run(False)
    dev, calls = run(True)
    assert len(calls) == iters + 1
    for eks in (host, dev):
        assert eks.Uall.shape == (iters + 1, 2, J) and eks.Gall.shape == (iters + 1, 25 + ns, J)
        assert np.all(np.isfinite(eks.Uall)) and np.all(np.isfinite(eks.Gall))
        assert isinstance(eks.W0, np.ndarray) and eks.W0.shape == (ns, J) and eks.W0.dtype == np.float64
        assert np.array_equal(eks.W0, eks.Gall[-1][25:]) and np.array_equal(eks.Gstar, eks.Gall[-1][:25])
        assert np.array_equal(eks.Ustar, eks.Uall[-1]) and len(eks.metrics["t"]) == iters
        assert not hasattr(eks, "Wall")
    # iteration 0: every particle starts from wt; the envelope of that evaluation, from the host alone
    m = lc.make_model(name, shape, T=T, device=False)
    env = 0.0
    for j in range(0, J, 8):
        clean = lc.host_run(m, wt, t, tuple(ref["U"][:, j]))
        for seed in (1, 2, 3, 4):
            r = lc.host_run(m, wt, t, tuple(ref["U"][:, j]), noise_seed=seed)
            env = max(env, np.abs(np.r_[r["stats"], r["end"]] - np.r_[clean["stats"], clean["end"]]).max()
                      / np.abs(np.r_[clean["stats"], clean["end"]]).max())
    assert env <= lc.ENV_MAX
    scale = np.abs(host.Gall[0]).max()
    tol = (4 * env + 64 * lc.EPS) * scale
    dG = np.abs(dev.Gall[0] - host.Gall[0]).max()
    # the update is a smooth map of (U, G): its gain from G to U_next is bounded by |U_next - U| / |G - y| of this very step
    # times the condition of the moments; 1e3 covers it at these sizes with room (the step moves U by O(1), G - y is O(1))
    dU = np.abs(dev.Uall[1] - host.Uall[1]).max()
    print("pde run: env %.2e dG %.2e tol %.2e dU %.2e" % (env, dG, tol, dU))
    assert np.array_equal(dev.Uall[0], host.Uall[0])
    assert dG <= tol
    assert dU <= 1e3 * tol * max(1.0, np.abs(host.Uall[1]).max() / scale)

    keep, _ = run(True, update_wt=False)
    assert np.array_equal(keep.W0, np.tile(wt, J).reshape(J, ns).T)
    assert not np.array_equal(keep.Gall[-1][25:], keep.W0)           # the trace still holds each evaluation's end states

    lib, calls = run(True, ws=np.tile(wt, (4, 1)))
    assert not calls and len(lib.Wall) == iters + 1                  # the library draw keeps the plain loop


def test_long_window_in_distribution():
    """T = 4 with a spin-up and one kept window of 20 samples, fixed parameters, 1024 particles from perturbed starts: per
    statistic the device's ensemble mean against the host's 64-particle mean of the fixture (tools/make_l96_fixture.py)
    within 5 standard errors of the difference.  Seeds are fixed: the verdict is deterministic."""
    import make_l96_fixture as fx
    gold = np.load(GOLDEN)
    m = fx.model(device=True)
    t = fx.times()
    J = 1024
    starts = fx.starts(J, seed=fx.DEVICE_SEED)
    U = np.tile(lc.PAR_MEAN[:, None], (1, J))
    eng = _engine(4, 25, J, "float64")
    G, W, info = _apply(m, eng, U, starts, t)
    assert np.all(info[0] == 0) and np.all(np.isfinite(G)) and np.all(np.isfinite(W))
    mean, sd = G.mean(axis=1), G.std(axis=1, ddof=1)
    bound = 5.0 * np.sqrt(gold["sd"] ** 2 / gold["n"] + sd ** 2 / J)
    print("long window: worst |dmean| / bound = %.3f" % (np.abs(mean - gold["mean"]) / bound).max())
    assert np.all(np.abs(mean - gold["mean"]) <= bound)
