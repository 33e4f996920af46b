"""Host forward models with carried state, the Lorenz family.

``sampling.run`` drives two kinds of forward maps (ces/calibrate.py:342-353):
``type == 'map'`` (one call per particle, ces/utils.py:5-122) and ``type ==
'pde'`` (an ODE solved per particle from a carried state, then summarised into
observables: ces/calibrate.py:132-168 and ces/utils.py:124-455).  These are host
code in the reference and the default here (BASELINE.json north_star); the
Lorenz '63 pair and the two-scale Lorenz '96 family also offer the whole ensemble on the device
(``set_solver(device=True)`` -> ``forward_pde_device``, cesx_lorenz_three_* / cesx_lorenz_*), which ``sampling.run`` and
``MCMC.model_mh(chains=)`` take.  The classes keep the reference's names,
attributes, call conventions and default arguments so that its notebooks
(examples/notebooks/{linear,lorenz63}.ipynb) run against ``ces_amd.calibrate``
unchanged; the right-hand sides are written in vectorised numpy rather than
per-variable Python loops.  ``lineal_log``, ``elliptic`` and ``banana`` of
ces/utils.py are closed-form maps, not models with carried state: they live in
ces_amd/utils.py beside ``lineal`` (with their device hook and, for the last two,
a fused chain kernel), not here.

Parity: every class is checked against outputs of the reference's own
``ces/utils.py`` (it imports unmodified in the build container) stored in
tests/golden/models.npz by oracle/make_golden_models.py.
"""
import numpy as np

from .utils import lineal


class lorenz63(object):
    """Lorenz '63 with (r, b) as parameters, sigma = 10 fixed (ces/utils.py:124-194).

    ``solve`` integrates with ``scipy.integrate.odeint`` over the time vector the driver
    passes (ces/calibrate.py:145) -- with ``solve_ivp`` once ``set_solver`` (build-only) has been
    called; ``statistics`` returns the 9 first and second moments
    over the LAST window of ``l_window * freq`` samples (the sample at t[0] is dropped,
    ces/utils.py:191-193)."""

    def __init__(self, l_window=10, freq=100):
        self.n_state = 3
        self.n_obs = 9
        self.l_window = l_window
        self.freq = freq
        self.solve_init = False
        self.model_name = "lorenz63"
        self.type = "pde"

    def __repr__(self):
        return self.model_name

    def __str__(self):
        return self.model_name + str(self.n_state)

    def model(self, w, t, sigma=10., r=28., b=8. / 3):
        x, y, z = w
        return [sigma * (y - x), r * x - y - x * z, x * y - b * z]

    def __call__(self, w, t, r=28., b=8. / 3):
        return self.model(w, t, 10., r, b)

    def set_solver(self, method="RK45", dt=np.inf, rtol=1e-3, atol=1e-6, device=False):
        """Build-only (the reference has none): after a call ``solve`` integrates with ``scipy.integrate.solve_ivp`` over
        ``[t[0], t[-1]]`` (``max_step=dt``) instead of ``odeint``.  ``device=True``: the model also offers
        ``forward_pde_device``, the whole ensemble integrated on the device (cesx_lorenz_three_*,
        ces_amd/csrc/kernels_l63.hip: scipy's RK45 restated, one particle per lane).  ``solve`` and ``statistics`` stay the
        host path either way."""
        if device and method != "RK45":
            raise ValueError("lorenz63.set_solver: device=True integrates with RK45 only, not %r" % (method,))
        self.method, self.dt, self.rtol, self.atol = method, dt, rtol, atol
        self.solve_init = True
        if device:
            self.forward_pde_device = self._forward_pde_device
        else:
            self.__dict__.pop("forward_pde_device", None)

    def solve(self, w0, t, args=()):
        from scipy import integrate
        if not self.solve_init:
            return integrate.odeint(self, w0, t, args=args)
        return integrate.solve_ivp(lambda tt, y: self(y, tt, *args), [t[0], t[-1]], w0, t_eval=t, method=self.method,
                                   max_step=self.dt, rtol=self.rtol, atol=self.atol).y.T

    def statistics(self, ws):
        x, y, z = ws[:, 0], ws[:, 1], ws[:, 2]
        feats = np.stack([x, y, z, x * x, y * y, z * z, x * y, x * z, y * z])
        win = int(self.l_window * self.freq)
        # adjacent windows over samples 1.. ; the last one is the observable
        return feats[:, 1:].reshape(self.n_obs, -1, win).mean(axis=2)[:, -1]

    # ---- build-only hook: the whole ensemble on the device (cesx_lorenz_three_*) ----
    n_params = 2
    DEVICE_PAR_ROW = (-1, 0, 1)                        # the row of U each of (sigma, r, b) is read from, or -1 ...
    DEVICE_PAR_FIXED = (10., 0., 0.)                   # ... and its fixed value (``__call__`` passes sigma = 10)
    DEVICE_PAR_LOG = (0, 0, 0)                         # 1: the row holds the parameter's logarithm
    device_max_attempts = 1000000                      # attempted steps after which a particle ends with status 3

    def device_descriptor(self, t, p=None, n_obs=None):
        """What cesx_lorenz_three_set takes (include/cesx.h), as a dict built in numpy.  ``ValueError`` with the reason
        wherever only the host path (``solve`` + ``statistics``, enka.G_pde_ens) applies."""
        host = "; integrate on the host (model.solve, enka.G_pde_ens) instead"
        if "forward_pde_device" not in self.__dict__:
            raise ValueError("lorenz63 forward_pde_device: set_solver(device=True) has not been called" + host)
        if self.method != "RK45":
            raise ValueError("lorenz63 forward_pde_device: method %r is not RK45" % (self.method,) + host)
        if t is None:
            raise ValueError("lorenz63 forward_pde_device: no sample times t" + host)
        t = np.asarray(t, dtype=np.float64).reshape(-1)
        if n_obs is not None and int(n_obs) != 9:
            raise ValueError("lorenz63 forward_pde_device: the model's n_obs = 9 differs from the engine's n_obs = %d"
                             % (n_obs,) + host)
        if p is not None and int(p) != self.n_params:
            raise ValueError("lorenz63 forward_pde_device: the model's p = %d differs from the engine's p = %d"
                             % (self.n_params, p) + host)
        dt, rtol, atol = float(self.dt), float(self.rtol), float(self.atol)
        if not dt > 0 or not (rtol > 0 and np.isfinite(rtol)) or not (atol > 0 and np.isfinite(atol)):
            raise ValueError("lorenz63 forward_pde_device: dt = %r, rtol = %r and atol = %r must be positive"
                             % (self.dt, self.rtol, self.atol) + host)
        if t.size < 2 or not np.all(np.isfinite(t)) or np.any(np.diff(t) <= 0):
            # (solve_ivp: "Values in t_eval are not properly sorted")
            raise ValueError("lorenz63 forward_pde_device: t must increase" + host)
        win = int(self.l_window * self.freq)
        if win != self.l_window * self.freq or win < 1:
            raise ValueError("lorenz63 forward_pde_device: l_window * freq must be a whole sample count" + host)
        if t.size - 1 < win or (t.size - 1) % win:
            # (the reshape of ``statistics`` raises there)
            raise ValueError("lorenz63 forward_pde_device: the %d samples after the first do not fill whole windows of %d"
                             % (t.size - 1, win) + host)
        return dict(n_obs=9, p=int(self.n_params), par_row=np.asarray(self.DEVICE_PAR_ROW, dtype=np.int32),
                    par_fixed=np.asarray(self.DEVICE_PAR_FIXED, dtype=np.float64),
                    par_log=np.asarray(self.DEVICE_PAR_LOG, dtype=np.int32),
                    t0=float(t[0]), T=float(t[-1]), max_step=dt, rtol=rtol, atol=atol, t=t,
                    window_samples=win, max_attempts=int(self.device_max_attempts))

    def _fingerprint(self, t):
        return (type(self).__name__, tuple(self.DEVICE_PAR_ROW), tuple(float(v) for v in self.DEVICE_PAR_FIXED),
                tuple(self.DEVICE_PAR_LOG), self.method, float(self.dt), float(self.rtol), float(self.atol),
                float(self.l_window), float(self.freq), int(self.device_max_attempts),
                np.asarray(t, dtype=np.float64).tobytes())

    def invalidate_device(self):
        """Forget the map installed in an engine: the next ``forward_pde_device`` builds and installs the descriptor again."""
        self._dev_fp = None
        self._dev_token = 0

    def ensure_installed(self, engine, t):
        """Make THIS model the Lorenz '63 map installed in ``engine``: installed once, again when any field of the descriptor
        changed or another model installed its own on the same engine (``invalidate_device()`` forces it)."""
        fp = self._fingerprint(t)
        if (getattr(self, "_dev_fp", None) != fp
                or getattr(engine, "_l63_token", None) is not getattr(self, "_dev_token", 0)):
            desc = self.device_descriptor(t, engine.p, engine.n_obs)
            self._dev_token = engine.l63_set(desc)
            self._dev_fp = fp

    def _forward_pde_device(self, engine, U_dev, W_dev, t, out=None, W_out=None, check=True):
        """(G (9, J), W_next (3, J) fp64) on the device: every column of ``U_dev`` integrated from its column of ``W_dev``
        over ``t`` (what enka.G_pde does per particle).  ``check`` (default): read the status words -- synchronises -- and
        raise ``ValueError`` naming the first particle that failed.  ``check=False`` reads nothing back: a failed particle's
        outputs are NaN (``MCMC.model_mh(chains=)`` rejects such a proposal)."""
        self.ensure_installed(engine, t)
        G, W_next, info = engine.l63_apply(U_dev, W_dev, out=out, W_out=W_out)
        if check:
            status = info[0].cpu().numpy()
            bad = np.flatnonzero(status)
            if bad.size:
                from .engine import L63_STATUS
                j = int(bad[0])
                raise ValueError("lorenz63 forward_pde_device: particle %d failed with status %d: %s"
                                 % (j, status[j], L63_STATUS.get(int(status[j]), "unknown")))
        return G, W_next


class lorenz63_log(lorenz63):
    """Same system in (log r, log b) (ces/utils.py:196-227)."""

    def __init__(self, l_window=10, freq=100):
        super().__init__(l_window=l_window, freq=freq)
        self.model_name = "lorenz63_log"

    def model(self, w, t, sigma=10., log_r=np.log(28.), log_b=np.log(8. / 3)):
        return super().model(w, t, sigma, np.exp(log_r), np.exp(log_b))

    def __call__(self, w, t, log_r=np.log(28.), log_b=np.log(8. / 3)):
        return self.model(w, t, 10., log_r, log_b)

    DEVICE_PAR_LOG = (0, 1, 1)                         # r = exp(U[0]), b = exp(U[1])

    def grad_logjacobian(self, params):
        return -np.exp(-params)

    def logjacobian(self, params):
        return -params.sum(axis=0)


def _l96_rhs(X, n_slow, n_fast, h, F, c, b):
    """Two-scale Lorenz '96 tendencies (ces/utils.py:279-297), vectorised with cyclic shifts:
    dX_k = -X_{k-1}(X_{k-2} - X_{k+1}) - X_k + F - h c mean_l(Y_{l,k}),
    dY_j = -c b Y_{j+1}(Y_{j+2} - Y_{j-1}) - c Y_j + (h c / n_fast) X_{j // n_fast}."""
    Y = X[n_slow:]
    X = X[:n_slow]
    dX = (-np.roll(X, 1) * (np.roll(X, 2) - np.roll(X, -1)) - X + F
          - (h * c) * Y.reshape(n_slow, n_fast).mean(axis=1))
    dY = (-c * b * np.roll(Y, -1) * (np.roll(Y, -2) - np.roll(Y, 1)) - c * Y
          + ((h * c) / n_fast) * np.repeat(X, n_fast))
    return np.hstack((dX, dY))


class lorenz96(object):
    """Two-scale Lorenz '96, parameters (h, F, log c, b) (ces/utils.py:229-343)."""

    n_params = 4

    def __init__(self, n_slow=36, n_fast=10, l_window=10, freq=10, spinup=10):
        self.n_slow = n_slow
        self.n_fast = n_fast
        self.n_state = self.n_slow * (self.n_fast + 1)
        self.l_window = l_window
        self.freq = freq
        self.spinup = spinup
        self.solve_init = False
        self.model_name = "lorenz96"
        self.type = "pde"

    def __repr__(self):
        tail = "" if self.n_params == 4 else "," + str(self.n_params)
        return self.model_name + "," + str(self.n_slow) + "," + str(self.n_fast) + tail

    def __str__(self):
        print("Model: ..................... Lorenz 96")
        print("Number of slow variables ... %s" % (self.n_slow))
        print("Number of fast variables ... %s" % (self.n_fast))
        print("Number of parameters........ %s" % (self.n_params))
        print("Solver initialized ......... %s" % (self.solve_init))
        return str()

    def model(self, X, t, h=1., F=10., log_c=np.log(10.), b=10.):
        return _l96_rhs(np.asarray(X), self.n_slow, self.n_fast, h, F, np.exp(log_c), b)

    def __call__(self, t, w, h=1., F=10., log_c=np.log(10.), b=10.):
        return self.model(w, t, h, F, log_c, b)

    def generate_initial(self):
        """Slow variables ~ U(-5, 10); every fast variable starts at its slow variable."""
        x = np.random.rand(self.n_slow) * 15 - 5
        return np.concatenate([x, np.repeat(x, self.n_fast)])

    def set_solver(self, method="RK45", T=20, dt=0.1, device=False):
        """``device=True`` (build-only): the model also offers ``forward_pde_device``, the whole ensemble integrated on the
        device (cesx_lorenz_*, ces_amd/csrc/kernels_l96.hip: scipy's RK45 restated, one wave per particle).  ``solve`` and
        ``statistics`` stay the host path either way."""
        if device and method != "RK45":
            raise ValueError("lorenz96.set_solver: device=True integrates with RK45 only, not %r" % (method,))
        self.method, self.dt, self.T = method, dt, T
        self.solve_init = True
        if device:
            self.forward_pde_device = self._forward_pde_device
        else:
            self.__dict__.pop("forward_pde_device", None)

    def solve(self, w0, t, args=()):
        from scipy import integrate
        if not self.solve_init:
            raise TypeError("lorenz96.solve: call set_solver first")   # the reference fails in np.empty() here
        res = integrate.solve_ivp(fun=lambda tt, y: self(tt, y, *args), t_span=[0, self.T], y0=w0,
                                  t_eval=t, method=self.method, max_step=self.dt)
        return res.y.T

    def _phi(self, ws):
        """5 blocks of n_slow window means: X, X^2, mean_l Y, mean_l Y^2, X mean_l Y
        (ces/utils.py:331-341); columns = adjacent windows after the spin-up."""
        ws = ws.T
        win = self.l_window * self.freq
        data = ws[:, (self.spinup * self.freq + 1):].reshape(self.n_state, -1, win)
        X = data[:self.n_slow]
        Y = data[self.n_slow:].reshape(self.n_slow, self.n_fast, -1, win)
        Ybar = Y.mean(axis=1)
        return np.vstack([X.mean(axis=2), (X ** 2).mean(axis=2), Ybar.mean(axis=2),
                          (Y ** 2).mean(axis=1).mean(axis=2), (X * Ybar).mean(axis=2)])

    def statistics(self, ws):
        return self._phi(ws)[:, -1]

    # ---- build-only hook: the whole ensemble on the device (cesx_lorenz_*) ----
    DEVICE_PAR_ROW = (0, 1, 2, 3)                      # the row of U each of (h, F, log c, b) is read from, or -1 ...
    DEVICE_PAR_FIXED = (0.0, 0.0, 0.0, 0.0)            # ... and its fixed value (the subclasses' ``__call__`` defaults)
    DEVICE_MAX_STATE = 448
    DEVICE_RTOL, DEVICE_ATOL = 1e-3, 1e-6              # solve_ivp's defaults: ``solve`` passes neither
    device_max_attempts = 1000000                      # attempted steps after which a particle ends with status 3

    def _device_stat_mode(self):
        return 0

    def device_descriptor(self, t, p=None, n_obs=None):
        """What cesx_lorenz_set takes (include/cesx.h), as a dict built in numpy.  ``ValueError`` with the reason wherever
        only the host path (``solve`` + ``statistics``, enka.G_pde_ens) applies."""
        host = "; integrate on the host (model.solve, enka.G_pde_ens) instead"
        if "forward_pde_device" not in self.__dict__:
            raise ValueError("lorenz96 forward_pde_device: set_solver(device=True) has not been called" + host)
        if self.method != "RK45":
            raise ValueError("lorenz96 forward_pde_device: method %r is not RK45" % (self.method,) + host)
        if t is None:
            raise ValueError("lorenz96 forward_pde_device: no sample times t" + host)
        t = np.asarray(t, dtype=np.float64).reshape(-1)
        n_slow, n_fast = int(self.n_slow), int(self.n_fast)
        if n_slow != self.n_slow or n_fast != self.n_fast or n_slow < 4 or n_fast < 1:
            raise ValueError("lorenz96 forward_pde_device: n_slow = %r < 4 or n_fast = %r < 1" % (self.n_slow, self.n_fast) + host)
        if n_slow * (n_fast + 1) > self.DEVICE_MAX_STATE:
            raise ValueError("lorenz96 forward_pde_device: n_state = %d > %d is not supported on the device"
                             % (n_slow * (n_fast + 1), self.DEVICE_MAX_STATE) + host)
        mode = self._device_stat_mode()
        if mode == 2 and n_slow < 8:
            raise ValueError("lorenz96 forward_pde_device: hom = False reads slow index 7, n_slow = %d" % n_slow + host)
        mine = 5 * n_slow if mode == 0 else 5
        if n_obs is not None and int(n_obs) != mine:
            raise ValueError("lorenz96 forward_pde_device: the model's n_obs = %d differs from the engine's n_obs = %d"
                             % (mine, n_obs) + host)
        if p is not None and int(p) != self.n_params:
            raise ValueError("lorenz96 forward_pde_device: the model's p = %d differs from the engine's p = %d"
                             % (self.n_params, p) + host)
        T, dt = float(self.T), float(self.dt)
        if not (T > 0 and np.isfinite(T)) or not dt > 0:
            raise ValueError("lorenz96 forward_pde_device: T = %r and dt = %r must be positive" % (self.T, self.dt) + host)
        if t.size < 2 or not np.all(np.isfinite(t)) or np.any(np.diff(t) <= 0) or t[0] < 0 or t[-1] > T:
            # (solve_ivp: "Values in t_eval are not within t_span" / "not properly sorted")
            raise ValueError("lorenz96 forward_pde_device: t must increase within [0, T = %g]" % T + host)
        spin, win = int(self.spinup * self.freq), int(self.l_window * self.freq)
        if spin != self.spinup * self.freq or win != self.l_window * self.freq or spin < 0 or win < 1:
            raise ValueError("lorenz96 forward_pde_device: spinup * freq and l_window * freq must be whole sample counts" + host)
        rest = t.size - 1 - spin
        if rest < win or rest % win:
            # (the reshape of ``_phi`` raises there)
            raise ValueError("lorenz96 forward_pde_device: the %d samples after the spin-up do not fill whole windows of %d"
                             % (rest, win) + host)
        return dict(n_slow=n_slow, n_fast=n_fast, n_obs=mine, p=int(self.n_params), stat_mode=mode,
                    par_row=np.asarray(self.DEVICE_PAR_ROW, dtype=np.int32),
                    par_fixed=np.asarray(self.DEVICE_PAR_FIXED, dtype=np.float64),
                    T=T, max_step=dt, rtol=self.DEVICE_RTOL, atol=self.DEVICE_ATOL, t=t,
                    spinup_samples=spin, window_samples=win, max_attempts=int(self.device_max_attempts))

    def _fingerprint(self, t):
        return (type(self).__name__, int(self.n_slow), int(self.n_fast), int(self.n_params), self._device_stat_mode(),
                tuple(self.DEVICE_PAR_ROW), tuple(float(v) for v in self.DEVICE_PAR_FIXED), float(self.T), float(self.dt),
                self.method, float(self.spinup), float(self.l_window), float(self.freq), int(self.device_max_attempts),
                np.asarray(t, dtype=np.float64).tobytes())

    def invalidate_device(self):
        """Forget the map installed in an engine: the next ``forward_pde_device`` builds and installs the descriptor again."""
        self._dev_fp = None
        self._dev_token = 0

    def ensure_installed(self, engine, t):
        """Make THIS model the Lorenz '96 map installed in ``engine``: installed once, again when any field of the descriptor
        changed or another model installed its own on the same engine (``invalidate_device()`` forces it)."""
        fp = self._fingerprint(t)
        if (getattr(self, "_dev_fp", None) != fp
                or getattr(engine, "_l96_token", None) is not getattr(self, "_dev_token", 0)):
            desc = self.device_descriptor(t, engine.p, engine.n_obs)
            self._dev_token = engine.l96_set(desc)
            self._dev_fp = fp

    def _forward_pde_device(self, engine, U_dev, W_dev, t, out=None, W_out=None, check=True):
        """(G (n_obs, J), W_next (n_state, J) fp64) on the device: every column of ``U_dev`` integrated from its column of
        ``W_dev`` over ``t`` (what enka.G_pde does per particle).  ``ValueError`` names the first particle that failed --
        the exception the host path ends in (``statistics``' reshape of a truncated solution).  Reads the status words:
        synchronises.  ``check=False`` reads nothing back and raises nothing: a failed particle's outputs are NaN
        (``MCMC.model_mh(chains=)`` rejects such a proposal)."""
        self.ensure_installed(engine, t)
        G, W_next, info = engine.l96_apply(U_dev, W_dev, out=out, W_out=W_out)
        if check:
            status = info[0].cpu().numpy()
            bad = np.flatnonzero(status)
            if bad.size:
                from .engine import L96_STATUS
                j = int(bad[0])
                raise ValueError("lorenz96 forward_pde_device: particle %d failed with status %d: %s"
                                 % (j, status[j], L96_STATUS.get(int(status[j]), "unknown")))
        return G, W_next

    def grad_logjacobian(self, params):
        # as the reference computes it (ces/utils.py:343-347): the exponent is taken of the zero it
        # has just written, so the third entry is -1
        out = np.zeros_like(params)
        out[2] = -np.exp(-out[2])
        return out


class lorenz96_hom(lorenz96):
    """Statistics averaged over the slow index (homogeneous), ces/utils.py:349-367."""

    def __init__(self):
        super().__init__()
        self.hom = True

    def statistics(self, ws):
        phi = self._phi(ws)[:, -1].reshape(5, -1)
        return phi.mean(axis=1) if self.hom else phi[:, 7]

    def _device_stat_mode(self):
        return 1 if self.hom else 2


class lorenz96Fc(lorenz96):
    """(F, log c) free, h = 1, b = 10 (ces/utils.py:369-389)."""
    n_params = 2

    def __init__(self):
        super().__init__()

    def __call__(self, t, w, F=10., log_c=np.log(10.)):
        return self.model(w, t, 1., F, log_c, 10.)

    DEVICE_PAR_ROW = (-1, 0, 1, -1)
    DEVICE_PAR_FIXED = (1., 0., 0., 10.)


class lorenz96Fb(lorenz96):
    """(F, b) free (ces/utils.py:391-408)."""
    n_params = 2

    def __call__(self, t, w, F=10., b=10.):
        return self.model(w, t, 1., F, np.log(10), b)

    DEVICE_PAR_ROW = (-1, 0, -1, 1)
    DEVICE_PAR_FIXED = (1., 0., np.log(10), 0.)


class lorenz96hFb(lorenz96):
    """(h, F, b) free (ces/utils.py:410-428)."""
    n_params = 3

    def __call__(self, t, w, h=1., F=10., b=10.):
        return self.model(w, t, h, F, np.log(10), b)

    DEVICE_PAR_ROW = (0, 1, -1, 2)
    DEVICE_PAR_FIXED = (0., 0., np.log(10), 0.)


class lorenz96hcb(lorenz96):
    """(h, log c, b) free (ces/utils.py:430-448)."""
    n_params = 3

    def __call__(self, t, w, h=1., log_c=np.log(10.), b=10.):
        return self.model(w, t, h, 10., log_c, b)

    DEVICE_PAR_ROW = (0, -1, 1, 2)
    DEVICE_PAR_FIXED = (0., 10., 0., 0.)


def lorenz96_dim(t, X, h=1., F=10., c=2 ** 7., b=1.):
    """Dimensional two-scale Lorenz '96 with fixed coupling 0.8 (ces/utils.py:450-466)."""
    n_slow, n_fast = 36, 10
    Y = X[n_slow:]
    X = X[:n_slow]
    dX = -np.roll(X, 1) * (np.roll(X, 2) - np.roll(X, -1)) - X + F - 0.8 * Y.reshape(n_slow, n_fast).mean(axis=1)
    dY = -c * np.roll(Y, -1) * (np.roll(Y, -2) - np.roll(Y, 1)) - c * Y + c * np.repeat(X, n_fast)
    return np.hstack((dX, dY))
