"""Shared inputs and host references of the Lorenz '96 device map's tests (tests/test_gpu_l96.py, tests/test_l96_host.py).

A chaotic ODE under an adaptive controller cannot be compared pointwise over a long window, so the pointwise cases are
short (T = 0.2, 0.5) and their tolerance comes from the host alone:

* reference: scipy's ``RK45`` stepped exactly as ``solve_ivp(t_eval=t)`` steps it, on ``ces_amd.models`` (``host_run``;
  tests/test_l96_host.py checks once that this is ``model.solve`` bit for bit);
* envelope: the host rerun four times with every right-hand-side value multiplied by ``1 + 16 * 2**-53 * s``, s = +-1 from
  ``RandomState(1..4)`` -- about ten roundings of the right-hand side plus up to seven of the stage sum, which the device may
  do differently per component and stage.  ``env_j`` is the largest deviation from the clean run relative to the run's largest
  magnitude, separately for the end state and the statistics;
* bound: ``4 * env_j + 64 * 2**-53`` (the factor 4 covers correlated signs and the reductions), plus ``2**-23`` on the
  statistics of an fp32 engine, whose host reference gets the fp32-rounded parameters.  An envelope above 1e-6 means the case
  is mis-set-up.

Every reference is computed once per process and shared (``functools.lru_cache``); the arrays are handed out read-only.
"""
import functools

import numpy as np

EPS = 2.0 ** -53
NOISE = 16 * EPS
ENV_MAX = 1e-6
PAR_MEAN = np.array([1.0, 10.0, np.log(10.0), 10.0])
PAR_STD = np.array([0.3, 3.0, 0.3, 3.0])
J_MAX = 96            # the draws are made for exactly the largest ensemble of the pointwise cases (see ``inputs``)
CLASSES = ("lorenz96", "lorenz96_hom", "lorenz96Fc", "lorenz96Fb", "lorenz96hFb", "lorenz96hcb")
FIXED_SHAPE = ("lorenz96_hom", "lorenz96Fc")           # these call super().__init__() without arguments: (36, 10)


def make_model(name="lorenz96", shape=(5, 3), T=0.2, dt=0.1, device=True, l_window=1, freq=10, spinup=0):
    from ces_amd import models
    cls = getattr(models, name)
    if name in FIXED_SHAPE:
        m = cls()
        m.l_window, m.freq, m.spinup = l_window, freq, spinup
    else:
        m = cls(n_slow=shape[0], n_fast=shape[1], l_window=l_window, freq=freq, spinup=spinup)
    m.set_solver(T=T, dt=dt, device=device) if device else m.set_solver(T=T, dt=dt)
    return m


def model_shape(name, shape):
    return (36, 10) if name in FIXED_SHAPE else tuple(shape)


def times(T, n=21, t_last=None):
    return np.linspace(0.0, T if t_last is None else t_last, n)


def _ro(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def attractor_state(n_slow, n_fast):
    """``generate_initial()`` (seed 1) integrated to T = 5 on the host at (1, 10, log 10, 10)."""
    from ces_amd import models
    m = models.lorenz96(n_slow=n_slow, n_fast=n_fast)
    m.set_solver(T=5, dt=0.1)
    state = np.random.get_state()
    np.random.seed(1)
    w0 = m.generate_initial()
    np.random.set_state(state)
    return _ro(m.solve(w0, np.array([0.0, 5.0]), args=tuple(PAR_MEAN))[-1].copy())


@functools.lru_cache(maxsize=None)
def inputs(n_slow, n_fast):
    """(params (4, J_MAX), starts (n_state, J_MAX)): particle j is the same whatever J a test takes.  One stream,
    RandomState(7): the parameters first, as one (4, J_MAX) block, then the elementwise start factors.  The layout matters at
    (4, 1), the most sensitive shape (c b up to 300 on a ring of four fast variables): of the layouts tried on the host --
    (4, 257), (257, 4), separate start seeds 8 .. 18 -- every one had particles among the first 96 whose envelope at T = 0.2
    exceeds the 1e-6 set-up limit (1.3e-6 .. 0.17); this one stays at 4.4e-7 (fp64 parameters) / 6.9e-7 (fp32-rounded)."""
    rs = np.random.RandomState(7)
    params = PAR_MEAN[:, None] + PAR_STD[:, None] * rs.standard_normal((4, J_MAX))
    w = attractor_state(n_slow, n_fast)
    starts = w[:, None] * (1.0 + 0.05 * rs.standard_normal((w.size, J_MAX)))      # elementwise
    return _ro(params), _ro(starts)


def class_rows(name):
    """The rows of the (h, F, log c, b) draw the class's parameter vector holds, in its own order."""
    from ces_amd import models
    row = getattr(models, name).DEVICE_PAR_ROW
    return [s for _, s in sorted((r, s) for s, r in enumerate(row) if r >= 0)]


def class_params(name, shape, dtype="float64"):
    """(U (p, J_MAX) as the engine of ``dtype`` sees it, widened back to float64; starts)."""
    params, starts = inputs(*model_shape(name, shape))
    U = params[class_rows(name)]
    return _ro(U.astype(dtype).astype(np.float64)), starts


def host_run(model, w0, t, args, noise_seed=None):
    """One particle as ``solve_ivp(fun, [0, T], w0, t_eval=t, method='RK45', max_step=dt)`` runs it (ivp.py:653-723), stepping
    the solver so that the accepted steps can be counted.  Returns dict(ws, stats, end, nfev, accepted, attempted, ok)."""
    from scipy.integrate import RK45
    if noise_seed is None:
        fun = lambda tt, y: model(tt, y, *args)                       # noqa: E731
    else:
        rs = np.random.RandomState(noise_seed)

        def fun(tt, y):
            f = model(tt, y, *args)
            return f * (1.0 + NOISE * (2.0 * rs.randint(0, 2, size=f.shape) - 1.0))
    solver = RK45(fun, 0.0, np.asarray(w0, dtype=np.float64), float(model.T), max_step=model.dt)
    ys, ti, acc = [], 0, 0
    while solver.status == "running":
        solver.step()
        if solver.status == "failed":
            break
        acc += 1
        inew = int(np.searchsorted(t, solver.t, side="right"))
        if inew > ti:
            ys.append(solver.dense_output()(t[ti:inew]))
            ti = inew
    ok = solver.status == "finished" and ti == t.size
    out = dict(nfev=solver.nfev, accepted=acc, attempted=(solver.nfev - 2) // 6, ok=ok, solver_status=solver.status)
    if ok:
        ws = np.hstack(ys).T
        out.update(ws=ws, stats=np.asarray(model.statistics(ws)), end=ws[-1])
    return out


@functools.lru_cache(maxsize=None)
def reference(name, shape, T, dtype, J, t_last=None):
    """Clean host run and envelope of the first ``J`` particles of (class, shape) at horizon ``T``: dict of read-only arrays
    G (n_obs, J), W (n_state, J), accepted / attempted (J,), env_G / env_W (J,), scale_G / scale_W (J,), nfev_moved (J,)."""
    m = make_model(name, shape, T=T, device=False)
    t = times(T, t_last=t_last)
    U, starts = class_params(name, shape, dtype)
    cols = {k: [] for k in ("G", "W", "accepted", "attempted", "env_G", "env_W", "scale_G", "scale_W", "nfev_moved")}
    for j in range(J):
        clean = host_run(m, starts[:, j], t, tuple(U[:, j]))
        assert clean["ok"], (name, shape, j, clean["solver_status"])
        sG, sW = np.abs(clean["stats"]).max(), np.abs(clean["end"]).max()
        eG = eW = 0.0
        moved = 0
        for seed in (1, 2, 3, 4):
            r = host_run(m, starts[:, j], t, tuple(U[:, j]), noise_seed=seed)
            assert r["ok"]
            moved += int(r["nfev"] != clean["nfev"])
            eG = max(eG, np.abs(r["stats"] - clean["stats"]).max() / sG)
            eW = max(eW, np.abs(r["end"] - clean["end"]).max() / sW)
        for k, v in (("G", clean["stats"]), ("W", clean["end"]), ("accepted", clean["accepted"]),
                     ("attempted", clean["attempted"]), ("env_G", eG), ("env_W", eW), ("scale_G", sG), ("scale_W", sW),
                     ("nfev_moved", moved)):
            cols[k].append(v)
    out = {k: _ro(np.asarray(v).T if k in ("G", "W") else np.asarray(v)) for k, v in cols.items()}
    out["t"], out["U"], out["W0"] = _ro(t), U[:, :J], starts[:, :J]
    return out


def tolerances(ref, dtype):
    """(tol_G (J,), tol_W (J,)) in absolute terms: (4 env_j + 64 * 2**-53) of the run's largest magnitude, + 2**-23 on the
    statistics of an fp32 engine (their storage rounding)."""
    tG = (4.0 * ref["env_G"] + 64 * EPS + (2.0 ** -23 if dtype == "float32" else 0.0)) * ref["scale_G"]
    tW = (4.0 * ref["env_W"] + 64 * EPS) * ref["scale_W"]
    return tG, tW


def check_against(ref, dtype, G, W, info, cols=None, counts=True):
    """The device's (G, W, info) for the particles ``cols`` of ``ref`` (default: the first G.shape[1]) within the envelope;
    step counts equal in all but 2 % of the particles, which must still agree within 1e-3 of the scale.  Returns the figures."""
    G, W, info = np.asarray(G, dtype=np.float64), np.asarray(W), np.asarray(info)
    cols = np.arange(G.shape[1]) if cols is None else np.asarray(cols)
    assert float(ref["env_G"][cols].max()) <= ENV_MAX and float(ref["env_W"][cols].max()) <= ENV_MAX, "mis-set-up case"
    assert np.array_equal(info[0], np.zeros(cols.size, dtype=info.dtype)), info[0]
    tG, tW = tolerances(ref, dtype)
    eG = np.abs(G - ref["G"][:, cols]).max(axis=0)
    eW = np.abs(W - ref["W"][:, cols]).max(axis=0)
    same = np.ones(cols.size, dtype=bool)
    if counts:
        same = (info[1] == ref["accepted"][cols]) & (info[2] == ref["attempted"][cols])
    fig = dict(worst_G=float((eG / tG[cols]).max()), worst_W=float((eW / tW[cols]).max()), differ=int((~same).sum()),
               env_G=float(ref["env_G"][cols].max()), env_W=float(ref["env_W"][cols].max()))
    print("l96 check:", fig)
    assert (~same).sum() <= 0.02 * cols.size, fig
    assert np.all(eG[same] <= tG[cols][same]), fig
    assert np.all(eW[same] <= tW[cols][same]), fig
    assert np.all(eG[~same] <= 1e-3 * ref["scale_G"][cols][~same]) and np.all(eW[~same] <= 1e-3 * ref["scale_W"][cols][~same]), fig
    return fig
