"""Forward maps evaluated in closed form (ces/utils.py:5-122).

``lineal`` is the forward map of the path BASELINE.json names (configs 1-3); ``lineal_log``, ``elliptic`` and ``banana``
(ces/utils.py:33-122) are the maps of the reference's linear.ipynb and elliptic.ipynb.  All four offer the build-only
device hook ``forward_device(engine, U_dev, out=None)``: ``lineal`` through the map installed in the engine
(cesx_forward_*), the other three through the engine's map stage (cesx_map_*, ces_amd/csrc/kernels_maps.hip; ``lineal_log``
as exp(U) into an engine-owned buffer, then its installed lineal map).  ``elliptic`` and ``banana`` also have a fused chain
kernel (cesx_mh_run_map: K Metropolis steps per launch), which ``MCMC.model_mh(chains=M)`` takes.  The other forward models
of ces/utils.py live in ces_amd/models.py and are re-exported here, so that
``import ces_amd.utils as utils`` offers what ``import ces.utils as utils`` does.
"""
import numpy as np


class lineal(object):
    """Linear forward map ``A theta + b`` (ces/utils.py:5-31): same attributes
    (``A, b, n_obs, flag_noise, noise_sigma, model_name, type``) and call
    convention, one parameter vector per call as enka.G_ens uses it
    (ces/calibrate.py:123-130)."""

    engine_lineal = True       # build-only: forward_device evaluates G = A U + b with the map installed in the engine

    def __init__(self, A, b=0, flag_noise=False):
        self.A = A
        self.b = b
        self.n_obs = A.shape[0]
        self.flag_noise = flag_noise
        self.noise_sigma = np.sqrt(0.1)
        self.model_name = "lineal"
        self.type = "map"

    def __repr__(self):
        return self.model_name

    def __call__(self, theta):
        out = np.matmul(self.A, theta) + self.b
        if self.flag_noise:
            out = out + self.noise_sigma * np.random.normal()
        return out

    def _fingerprint(self):
        out = []
        for a in (self.A, self.b):
            a = np.asarray(a)
            flat = a.reshape(-1)
            out.append((a.shape, a.dtype.str, flat[::max(1, flat.size // 64)].tobytes(), float(flat.sum()) if flat.size else 0.0))
        return tuple(out)

    def invalidate_device(self):
        """Forget the map installed in an engine (build-only): the next ``forward_device`` uploads A and b again."""
        self._dev_A = self._dev_b = self._dev_fp = None
        self._dev_token = 0

    # build-only hook: evaluate the whole shard on device
    def forward_device(self, engine, U_dev, out=None):
        if self.flag_noise:
            raise ValueError("the device hook evaluates the noise-free map only")
        # The map is installed in the engine once (cesx_forward_set_lineal: the engine keeps A and b in the layout of
        # its LDS-DMA update kernels) and applied every iteration (a per-call upload of a pageable host array cost
        # 9 ms per step at p = n_obs = 256, 20x the ensemble update itself).  An engine without the two-step entry
        # points (the CPU stand-in of the tests) takes the one-call form.
        if not hasattr(engine, "forward_set_lineal"):
            b = None
            if np.ndim(self.b) > 0 or self.b != 0:
                b = np.broadcast_to(np.asarray(self.b, dtype=np.float64), (self.n_obs,))
            return engine.forward_lineal(self.A, U_dev, b=b, out=out)
        self.ensure_installed(engine)
        return engine.forward_apply(U_dev, out=out)

    def ensure_installed(self, engine):
        """Make THIS map the one installed in ``engine`` (build-only).  Called by ``forward_device`` and -- before the moment
        kernels that read the installed map, cesx_moments_rest_lineal -- by ``ShardedUpdate.begin_lineal``: the G-dependent
        moments, G itself and K3 then all use the same map in every step (an edit of A or b between two steps, or another
        model that installed its map on the same engine, re-installs first)."""
        # the installed map is reused while A and b are THE SAME OBJECTS (strong references are kept, so an id cannot be
        # recycled) and a cheap fingerprint of their contents (shape, dtype, 64 strided samples, the sum) is unchanged:
        # an in-place edit of A or b between two calls re-installs the map.  ``invalidate_device()`` forces it.
        fp = self._fingerprint()
        if (getattr(self, "_dev_A", None) is not self.A or getattr(self, "_dev_b", None) is not self.b
                or getattr(self, "_dev_fp", None) != fp
                or getattr(engine, "_fwd_token", None) is not getattr(self, "_dev_token", 0)):
            b = None
            if np.ndim(self.b) > 0 or self.b != 0:
                b = np.broadcast_to(np.asarray(self.b, dtype=np.float64), (self.n_obs,))
            self._dev_token = engine.forward_set_lineal(np.asarray(self.A), b)      # (another model may have installed its map)
            self._dev_A, self._dev_b, self._dev_fp = self.A, self.b, fp

    _exp_params = False        # lineal_log: the map acts on exp(theta)

    def enable_gradient(self, leapfrog=False):
        """Offer the gradient of the map to ``MCMC.model_mh(update='langevin')`` (build-only, opt-in: without this call the
        instance has neither attribute and the sampler refuses it as before).  The instance gains

        ``jacobian(theta)``          on the host, (n_obs, p): ``A`` (``lineal_log``: ``A * exp(theta)[None, :]``)
        ``langevin_device(engine)``  with ``chains=M``: installs the map and hands A and b to the engine's adjoint images
                                     (cesx_mh_langevin_lineal_set), after which the Langevin step never forms a Jacobian: its
                                     gradient is an A^T product on the update kernels.
        ``leapfrog=True`` additionally marks the instance (``leapfrog_device = True``) for ``update='hmc'`` and ``adapt=``: the
        GEMM-form leapfrog of cesx_mh_hmc_lineal_* (kernels_hmclin.hip) on the same images.  Without it the mark is removed and
        the two are refused, as they were.  Returns ``self``."""
        if leapfrog not in (False, True):
            raise ValueError("enable_gradient: leapfrog must be False or True, got %r" % (leapfrog,))
        self.__dict__.pop("leapfrog_device", None)
        if leapfrog:
            self.leapfrog_device = True

        def jacobian(theta):
            A = np.asarray(self.A, dtype=np.float64)
            if not self._exp_params:
                return A.copy()
            return A * np.exp(np.asarray(theta, dtype=np.float64).reshape(-1))[None, :]

        def langevin_device(engine):
            self.ensure_installed(engine)
            b = None
            if np.ndim(self.b) > 0 or self.b != 0:
                b = np.broadcast_to(np.asarray(self.b, dtype=np.float64), (self.n_obs,))
            engine.mh_langevin_lineal_set(np.asarray(self.A, dtype=np.float64), b, exp_params=self._exp_params)

        self.jacobian = jacobian
        self.langevin_device = langevin_device
        return self


class _map_hook(object):
    """The device hook of the closed-form maps (build-only): one descriptor (``_map_desc``) installed in the engine's map
    stage (cesx_map_set), re-installed when a parameter changed or another model installed its own on the same engine."""

    map_kind = None            # 'elliptic' | 'banana' | 'exp' (ces_amd.engine.MAP_KINDS)
    fused_kind = False         # cesx_mh_run_map has an instantiation for this kind

    def _map_desc(self):
        raise NotImplementedError

    def _fingerprint(self):
        return (self.map_kind,) + tuple(float(v) for v in self._map_desc())

    def invalidate_device(self):
        """Forget the map installed in an engine (build-only): the next ``forward_device`` installs it again."""
        self._map_fp = None
        self._map_token = 0

    def ensure_installed(self, engine):
        """Make THIS model the one installed in the map stage of ``engine`` (build-only; ``invalidate_device()`` forces it)."""
        fp = self._fingerprint()
        if (getattr(self, "_map_fp", None) != fp
                or getattr(engine, "_map_token", None) is not getattr(self, "_map_token", 0)):
            self._map_token = engine.map_set(self.map_kind, self._map_desc())
            self._map_fp = fp

    def forward_device(self, engine, U_dev, out=None):
        if self.flag_noise:
            raise ValueError("the device hook evaluates the noise-free map only")
        self.ensure_installed(engine)
        return engine.map_apply(U_dev, out=out)

    def jacobian_device(self, engine, U_dev, out=None):
        """(G, DG) of the columns of ``U_dev`` on the device (build-only): float64 (n_obs, J) and (n_obs, p, J),
        ``DG[i][q] = dG_i / du_q`` as ``jacobian`` has it on the host (cesx_map_jac).  ``out``: a (G, DG) tuple."""
        if self.flag_noise:
            raise ValueError("the device hook evaluates the noise-free map only")
        self.ensure_installed(engine)
        return engine.map_jac(U_dev, out=out)


class lineal_log(lineal):
    """``A exp(phi) + b`` (ces/utils.py:33-51): ``lineal`` in log-parameters, with the log-Jacobian helpers."""

    engine_lineal = False      # G's moments do NOT follow from U's through A (ShardedUpdate.lineal_fast_ok): A acts on exp(U)
    map_kind = "exp"
    fused_kind = False
    _exp_params = True

    def __init__(self, A, flag_noise=False):
        super().__init__(A, flag_noise=flag_noise)
        self.model_name = "lineal_log"
        self.jacobian_adjusted = True

    def __call__(self, phi):
        return super().__call__(np.exp(phi))

    def grad_logjacobian(self, params):
        return -np.exp(-params)

    def logjacobian(self, params):
        if self.jacobian_adjusted:
            return -params.sum(axis=0)
        else:
            return 0.0

    def invalidate_device(self):
        super().invalidate_device()
        self._map_token = 0

    def ensure_installed(self, engine):
        """Both halves (build-only): the exp prologue in the engine's map stage -- ``map_set`` allocates the engine's
        (p, J) scratch buffer, never an apply -- and A, b as the installed lineal map (``_fingerprint`` is lineal's)."""
        if getattr(engine, "_map_token", None) is not getattr(self, "_map_token", 0):
            self._map_token = engine.map_set(self.map_kind, ())
        super().ensure_installed(engine)

    def forward_device(self, engine, U_dev, out=None):
        if self.flag_noise:
            raise ValueError("the device hook evaluates the noise-free map only")
        self.ensure_installed(engine)
        return engine.forward_apply(engine.map_apply(U_dev, out=engine.map_scratch), out=out)


class elliptic(_map_hook):
    """The two-point observation of the 1-d elliptic problem (ces/utils.py:53-89): ``p(x) = u2 x + exp(-u1)(-x^2/2 + x/2)``
    at ``x1 = 1/4`` and ``x2 = 3/4``.  ``__call__`` returns the LIST ``[x, y]`` as the reference does (``dG=True``: the
    2 x 2 Jacobian); ``theta`` is one particle or a (2, J) block."""

    map_kind = "elliptic"
    fused_kind = True

    def __init__(self, flag_noise=False):
        self.x1 = 1. / 4
        self.x2 = 3. / 4
        self.flag_noise = flag_noise
        self.sigma = np.sqrt(0.01)
        self.model_name = "elliptic"
        self.type = "map"

    def __repr__(self):
        return self.model_name

    def __str__(self):
        return self.model_name

    def __call__(self, theta, dG=False):
        u1, u2 = theta
        x = (u2 * self.x1) + (np.exp(-u1) * (-self.x1**2 + self.x1) * 0.5)
        y = (u2 * self.x2) + (np.exp(-u1) * (-self.x2**2 + self.x2) * 0.5)
        if self.flag_noise:                               # (:80-82: len(): a block of particles only)
            x += (self.sigma * np.random.normal(size=len(u1)))
            y += (self.sigma * np.random.normal(size=len(u2)))
        if dG:
            return np.array([[-np.exp(-u1) * (-self.x1**2 + self.x1) * 0.5, self.x1],
                             [-np.exp(-u1) * (-self.x2**2 + self.x2) * 0.5, self.x2]])
        return [x, y]

    def jacobian(self, theta):
        """``DG[i][q] = dG_i / dtheta_q`` (build-only name; the entries of ``__call__(theta, dG=True)``, :85-86): (2, 2) for
        one particle, (2, 2, J) for a (2, J) block, for which the reference's ``dG=True`` has no array to return."""
        u1, u2 = theta
        one = np.ones_like(np.asarray(u1, dtype=np.float64))
        return np.array([[-np.exp(-u1) * (-self.x1**2 + self.x1) * 0.5, self.x1 * one],
                         [-np.exp(-u1) * (-self.x2**2 + self.x2) * 0.5, self.x2 * one]])

    def _map_desc(self):
        return (self.x1, self.x2)


class banana(_map_hook):
    """The banana-shaped map ``(a u1, u2 / a - b (u1^2 + a^2))`` (ces/utils.py:91-122) with its correlated ``Gamma``.  One
    particle per call: the (2,) noise term is added -- times ``flag_noise`` -- whether or not noise is on, so the global
    RNG advances by two normals per call and a (2, J) block does not broadcast for J other than 2."""

    map_kind = "banana"
    fused_kind = True

    def __init__(self, a=1.0, b=.5, rho=.9, flag_noise=False):
        self.flag_noise = flag_noise
        self.sigma = np.sqrt(0.55)
        self.model_name = "banana"
        self.type = "map"
        self.a = a
        self.b = b
        self.Gamma = np.identity(2)
        self.Gamma[0, 1] = rho
        self.Gamma[1, 0] = rho
        self.Gamma = (0.55**2) * self.Gamma

    def __repr__(self):
        return self.model_name

    def __str__(self):
        return self.model_name

    def __call__(self, theta, dG=False):
        u1, u2 = theta
        x = u1 * self.a
        y = u2 / self.a - self.b * (u1**2 + self.a**2)
        return np.array([x, y]) + self.flag_noise * np.linalg.cholesky(self.Gamma).dot(np.random.normal(0, 1, [2, ]))

    def jacobian(self, theta):
        """``DG[i][q] = dG_i / dtheta_q = [[a, 0], [-2 b u1, 1 / a]]`` (build-only: the reference's ``banana`` takes ``dG`` and
        ignores it, as ``__call__`` here does): (2, 2) for one particle, (2, 2, J) for a (2, J) block."""
        u1, u2 = theta
        one = np.ones_like(np.asarray(u1, dtype=np.float64))
        return np.array([[self.a * one, 0.0 * one], [-2.0 * self.b * u1 * one, one / self.a]])

    def _map_desc(self):
        return (self.a, self.b)


def __getattr__(name):
    # re-export ces_amd.models lazily (it imports ``lineal`` from this module)
    from . import models
    try:
        return getattr(models, name)
    except AttributeError:
        raise AttributeError("module %r has no attribute %r" % (__name__, name)) from None


def hook_takes_out(hook):
    """Whether a model's ``forward_device(engine, U[, out=])`` hook accepts ``out=`` -- decided from its signature, once, not by
    catching ``TypeError`` around the call (a ``TypeError`` raised INSIDE a hook that does take ``out=`` would be swallowed and the
    forward map evaluated a second time through the copy fallback)."""
    import inspect
    try:
        prm = inspect.signature(hook).parameters
    except (TypeError, ValueError):
        return False
    return "out" in prm or any(q.kind is inspect.Parameter.VAR_KEYWORD for q in prm.values())
