"""Darcy-flow forward map on the host, in numpy/scipy.

The reference drives two MATLAB files through ``matlab.engine``
(``ces/darcy.py:9-138``); MATLAB is proprietary and absent here, so this module
restates their arithmetic:

* ``gaussrnd_coarse`` (utilities/mfiles/gaussrnd_coarse.m:6-23): KL
  coefficients ``N * tau^(alpha-1) (pi^2 |k|^2 + tau^2)^(-alpha/2) * xi`` with the
  constant mode removed, synthesised by MATLAB's ``idct2`` = orthonormal inverse
  2-D DCT-II (``scipy.fft.idctn(..., norm='ortho')``).
* ``solve_gwf`` (utilities/mfiles/solve_gwf.m:4-38): ``-div(exp(a) grad p) = 1`` on
  the unit square, ``p = 0`` on the boundary: cell-centred log-permeability is
  spline-interpolated to the K x K node grid (MATLAB ``interp2(...,'spline')`` =
  tensor-product not-a-knot cubic splines, which extrapolate to the boundary
  nodes), 5-point finite differences with arithmetic-mean face coefficients on
  the (K-2)^2 interior nodes, sparse solve, and spline interpolation of the
  pressure back to the cell centres.

Same classes and call conventions as the reference (``model``, ``model_trunc``,
``set_initial``, ``set_rank``, ``eval_rf``, ``solve_pde``, ``obs_index``);
``start`` / ``stop`` / ``set_rnd_seed`` are kept as no-ops so that
examples/scripts/darcy-flow.py:6-14 runs unchanged.

``__call__`` evaluates the map on the host, one particle per call, as the
reference does.  ``forward_device`` (build-only hook) evaluates the
same map for every column of a device-resident ensemble in one launch
(cesx_darcy_apply): everything but the solve is a
fixed linear operator or an elementwise ``exp``, so the host hands the engine the
matrices once (``device_descriptor``) and the kernel runs KL synthesis, the two
spline maps, the assembly and a banded LU with partial pivoting per particle, all
in fp64.  Two solvers, chosen with ``set_device_solver`` (build-only): ``'resident'``, the
default (ces_amd/csrc/kernels_darcy.hip, Nmesh 4..16: one particle's whole working
band in LDS), and ``'streamed'`` (ces_amd/csrc/kernels_darcy_stream.hip, Nmesh 4..64:
only the live window of the factorisation in LDS, the finished rows of U streamed
through an HBM workspace; ``device_max_workgroups`` bounds the grid and with it the
workspace, 0 = automatic).  With the hook ``sampling.run`` keeps a Darcy ensemble resident
(``noise='device'`` or ``xis=``) and ``MCMC.model_mh(chains=M)`` runs; the
default host flow is unchanged.  ``enable_gradient()`` (build-only, opt-in) adds the adjoint of the map: the operator is
symmetric, so the gradient of the data misfit is one more solve on the same factorisation -- ``jacobian`` and
``misfit_gradient`` on the host, ``gradient_device`` on the device (cesx_darcy_grad, ces_amd/csrc/kernels_darcy_grad.hip: the
resident solver only), and with ``jacobian`` the host path of ``MCMC.model_mh(update='langevin' / 'hmc', adapt=)``; with
``chains=M`` those updates run on ``gradient_device``: one adjoint launch per position, its gradient handed ready-made to the
Langevin and leapfrog entry points (cesx_mh_grad_source, ces_amd/csrc/kernels_darcy_chain.hip).

PARITY UNPINNED: the MATLAB reference cannot run here, so there is no golden
output; tests validate the restatement through the PDE itself (discrete
residual, manufactured solution, symmetry) rather than against the reference.
The device map is pinned to this host restatement, not to MATLAB.
"""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla
from scipy.fft import idctn
from scipy.interpolate import CubicSpline


def gaussrnd_coarse(xi, alpha, tau, N):
    """utilities/mfiles/gaussrnd_coarse.m:6-23.  ``xi``: (N, N) KL coefficients."""
    N = int(N)
    k = np.arange(N)
    K1, K2 = np.meshgrid(k, k)
    coef = tau ** (alpha - 1) * (np.pi ** 2 * (K1 ** 2 + K2 ** 2) + tau ** 2) ** (-alpha / 2)
    L = N * coef * np.asarray(xi, dtype=np.float64).reshape(N, N)
    L[0, 0] = 0.0
    return idctn(L, norm="ortho")


def _interp2_spline(x_src, z, x_dst):
    """MATLAB interp2(X, Y, Z, Xq, Yq, 'spline') on tensor grids with the same 1-D
    abscissae in both directions: not-a-knot cubic splines along each axis."""
    z = CubicSpline(x_src, z, axis=0, bc_type="not-a-knot", extrapolate=True)(x_dst)
    return CubicSpline(x_src, z, axis=1, bc_type="not-a-knot", extrapolate=True)(x_dst)


def assemble_gwf(a_nodes):
    """5-point operator of solve_gwf.m:19-35 for nodal coefficients ``a_nodes`` (K, K):
    returns the sparse matrix acting on the interior unknowns ordered column by column
    (MATLAB ``F(:)`` order), already scaled by (K-1)^2."""
    K = a_nodes.shape[0]
    m = K - 2
    c = a_nodes
    idx = lambda i, j: (j - 1) * m + (i - 1)          # interior node (i, j), 1-based interior indices
    rows, cols, vals = [], [], []
    for j in range(1, K - 1):
        for i in range(1, K - 1):
            diag = ((c[i - 1, j] + c[i, j]) / 2 + (c[i + 1, j] + c[i, j]) / 2
                    + (c[i, j - 1] + c[i, j]) / 2 + (c[i, j + 1] + c[i, j]) / 2)
            rows.append(idx(i, j)); cols.append(idx(i, j)); vals.append(diag)
            if i > 1:
                rows.append(idx(i, j)); cols.append(idx(i - 1, j)); vals.append(-(c[i - 1, j] + c[i, j]) / 2)
            if i < K - 2:
                rows.append(idx(i, j)); cols.append(idx(i + 1, j)); vals.append(-(c[i + 1, j] + c[i, j]) / 2)
            if j > 1:
                rows.append(idx(i, j)); cols.append(idx(i, j - 1)); vals.append(-(c[i, j - 1] + c[i, j]) / 2)
            if j < K - 2:
                rows.append(idx(i, j)); cols.append(idx(i, j + 1)); vals.append(-(c[i, j + 1] + c[i, j]) / 2)
    return sp.csc_matrix((vals, (rows, cols)), shape=(m * m, m * m)) * (K - 1) ** 2


def solve_gwf(coef):
    """utilities/mfiles/solve_gwf.m:4-38.  ``coef``: (K, K) log-permeability at cell
    centres; returns the pressure at the cell centres, (K, K)."""
    coef = np.asarray(coef, dtype=np.float64)
    K = coef.shape[0]
    centres = np.arange(1, 2 * K, 2) / (2.0 * K)       # 1/(2K) : 1/K : (2K-1)/(2K)
    nodes = np.linspace(0.0, 1.0, K)
    a = _interp2_spline(centres, np.exp(coef), nodes)
    A = assemble_gwf(a)
    rhs = np.ones((K - 2) * (K - 2))                    # spline of the constant 1 is 1
    x = spla.spsolve(A, rhs)
    P = np.zeros((K, K))
    P[1:-1, 1:-1] = x.reshape(K - 2, K - 2, order="F")  # x is in column-major (MATLAB F(:)) order
    # solve_gwf.m builds vec2mat(x, K-2) (= P^T), interpolates and transposes back; the grids
    # are the same in both directions, so that equals interpolating P itself
    return _interp2_spline(nodes, P, centres)


class model(object):
    """Full KL parametrisation, p = Nmesh^2 (ces/darcy.py:9-98)."""

    def __init__(self, alpha=2., tau=3., Nmesh=2. ** 4):
        self.alpha = alpha
        self.tau = tau
        self.Nmesh = Nmesh
        self.p = int(self.Nmesh * self.Nmesh)
        self.model_name = 'darcy-flow'
        self.type = 'map'

    def __call__(self, xi, full_solution=False):
        theta = self.eval_rf(xi)
        U = self.solve_pde(theta)
        if full_solution:
            return np.asarray(U).flatten()
        return np.asarray(U).flatten()[self.obs_index]

    # the MATLAB engine life cycle of ces/darcy.py:40-66 has no counterpart here
    def start(self, mpath=None):
        pass

    def stop(self):
        pass

    def set_rnd_seed(self, seed=1):
        pass

    def set_initial(self, seed=1):
        np.random.seed(seed)
        self.ustar = np.random.normal(0, 1, int(self.p))

    def set_rank(self):
        k = np.arange(int(self.Nmesh))
        K1, K2 = np.meshgrid(k, k)
        self.eigs = (self.tau ** (self.alpha - 1)) * (np.pi ** 2 * (K1 ** 2 + K2 ** 2) + self.tau ** 2) ** (-self.alpha / 2)
        self.eigs[0, 0] = 1e-10
        self.rank = (-self.eigs).flatten().argsort()

    def eval_rf(self, xi):
        return gaussrnd_coarse(np.asarray(xi, dtype=np.float64).reshape(int(self.Nmesh), -1),
                               self.alpha, self.tau, self.Nmesh)

    def solve_pde(self, theta):
        return solve_gwf(theta)

    # ---- build-only hook: the whole ensemble on the device (cesx_darcy_*) ----
    DEVICE_NMESH = (4, 16)     # not-a-knot needs four points; beyond 16 one particle's working band no longer fits in LDS
    DEVICE_NMESH_STREAMED = (4, 64)    # the streamed solver keeps only the live window in LDS (CESX_DARCY_STREAM_KMAX)
    DEVICE_SOLVERS = ("resident", "streamed")
    device_solver = "resident"
    device_max_workgroups = 0  # streamed: the largest grid an apply may launch (one workspace slot each); 0 = automatic

    def set_device_solver(self, kind):
        """Which kernel ``forward_device`` installs: ``'resident'`` (the default, Nmesh 4..16) or ``'streamed'`` (Nmesh 4..64).
        Part of the fingerprint: the next ``forward_device`` installs the map again."""
        if kind not in self.DEVICE_SOLVERS:
            raise ValueError("darcy set_device_solver: %r is neither 'resident' nor 'streamed'" % (kind,))
        if kind == "streamed" and hasattr(self, "gradient_device"):
            raise ValueError("darcy set_device_solver: the gradient of enable_gradient() is an adjoint solve on the factors the "
                             "resident solver keeps in LDS; the streamed solver does not keep its multipliers")
        self.device_solver = kind

    # ---- build-only: the adjoint of the map (opt-in, like ces_amd.utils.lineal.enable_gradient) ----
    def _operators(self):
        """(K, coef, D, S, R, scatter) of ``device_descriptor``, at any Nmesh >= 4 and without an ``obs_index``: the map as
        ``a = S exp(D (coef o Xi) D^T) S^T``, ``A(a) x = 1``, ``G = (R P R^T).flat[obs_index]``."""
        K = int(self.Nmesh)
        if K != self.Nmesh or K < 4:
            raise ValueError("darcy gradient: Nmesh = %r < 4 (or not an integer)" % (self.Nmesh,))
        key = self._fingerprint()
        if getattr(self, "_ops_key", None) == key:
            return self._ops
        self._ops_key, self._ops = key, self._build_operators(K)
        return self._ops

    def _build_operators(self, K):
        k = np.arange(K)
        K1, K2 = np.meshgrid(k, k)
        coef = K * (self.tau ** (self.alpha - 1) * (np.pi ** 2 * (K1 ** 2 + K2 ** 2) + self.tau ** 2) ** (-self.alpha / 2))
        coef[0, 0] = 0.0
        eye = np.eye(K)
        centres = np.arange(1, 2 * K, 2) / (2.0 * K)
        nodes = np.linspace(0.0, 1.0, K)
        return (K, coef, idctn(eye, axes=[0], norm="ortho"),
                CubicSpline(centres, eye, axis=0, bc_type="not-a-knot", extrapolate=True)(nodes),
                CubicSpline(nodes, eye, axis=0, bc_type="not-a-knot", extrapolate=True)(centres),
                np.asarray(self._device_scatter()).reshape(-1))

    def _adjoint(self, xi, weights, solver=None):
        """(G, d) for one particle: the map at the picked centres and ``d[:, t] = dG^T weights[:, t]``, (p, r) for ``weights``
        (n_obs, r), or a callable that forms them from G -- one sparse LU (``solver(A)`` returning a ``solve(rhs)``: the hook of the tests' banded restatement), the
        forward solve and r adjoint solves on it (A is symmetric).  The steps are those of include/cesx.h, cesx_darcy_grad."""
        K, coef, D, S, R, scatter = self._operators()
        m = K - 2
        obs = np.asarray(self.obs_index).reshape(-1)
        Xi = np.zeros(K * K)
        Xi[scatter] = np.asarray(xi, dtype=np.float64).reshape(-1)
        L = coef * Xi.reshape(K, K)
        L[0, 0] = 0.0
        e = np.exp(D @ L @ D.T)
        A = assemble_gwf(S @ e @ S.T)
        solve = spla.splu(A.tocsc()).solve if solver is None else solver(A)
        P = np.zeros((K, K))
        P[1:-1, 1:-1] = solve(np.ones(m * m)).reshape(m, m, order="F")
        G = (R @ P @ R.T).flatten()[obs]
        weights = np.asarray(weights(G) if callable(weights) else weights, dtype=np.float64).reshape(obs.size, -1)
        r = weights.shape[1]
        Z = np.zeros((r, K * K))
        for t in range(r):
            np.add.at(Z[t], obs, weights[:, t])
        W = R.T @ Z.reshape(r, K, K) @ R
        w = W[:, 1:-1, 1:-1].transpose(0, 2, 1).reshape(r, m * m)          # the interior, column-major unknowns
        lam = np.stack([solve(w[t]) for t in range(r)])
        Lam = np.zeros((r, K, K))
        Lam[:, 1:-1, 1:-1] = lam.reshape(r, m, m).transpose(0, 2, 1)
        da = np.zeros((r, K, K))
        fv = (Lam[:, 1:, :] - Lam[:, :-1, :]) * (P[1:, :] - P[:-1, :])      # a face between two boundary nodes gives 0 * 0
        fh = (Lam[:, :, 1:] - Lam[:, :, :-1]) * (P[:, 1:] - P[:, :-1])
        da[:, 1:, :] += fv
        da[:, :-1, :] += fv
        da[:, :, 1:] += fh
        da[:, :, :-1] += fh
        da *= -0.5 * (K - 1) ** 2
        dL = D.T @ (e * (S.T @ da @ S)) @ D
        d = (coef * dL).reshape(r, K * K)[:, scatter]
        d[:, scatter == 0] = 0.0
        return G, d.T

    def enable_gradient(self):
        """Offer the gradient of the map, to the host path of ``MCMC.model_mh(update='langevin' / 'hmc', adapt=)`` and to callers
        of their own (build-only, opt-in: without this call the instance has none of the attributes and the sampler refuses it
        as before; with ``chains=M`` the sampler runs on ``gradient_device``, one adjoint launch per position).  The 5-point operator is
        symmetric, so the adjoint solve is a second right-hand side of the forward solve's factorisation.  The instance gains

        ``jacobian(xi)``                          on the host, (n_obs, p): one sparse LU and n_obs adjoint solves
        ``misfit_gradient(xi, y, Gamma)``         on the host: (phi_d, d), phi_d = 1/2 r^T Gamma^{-1} r with r = G(xi) - y and
                                                  d = d phi_d / d xi (p,), from ONE adjoint solve
        ``gradient_device(engine, U_dev, out=None)``  (G, phi_d, d) of the columns of ``U_dev`` on the device, float64 (n_obs, J),
                                                  (J,) and (p, J), for the y and Gamma of the engine's ``set_problem``
                                                  (cesx_darcy_grad: the resident solver, Nmesh 4..16).  A particle whose system
                                                  is singular or not finite has NaN in all three; nothing is raised.
        ``ValueError`` with ``set_device_solver('streamed')``.  Returns ``self``."""
        if self.device_solver == "streamed":
            raise ValueError("darcy enable_gradient: the adjoint solve runs on the factors the resident solver keeps in LDS; the "
                             "streamed solver (set_device_solver('streamed')) does not keep its multipliers")

        def jacobian(xi):
            n = np.asarray(self.obs_index).size
            return self._adjoint(xi, np.eye(n))[1].T.copy()

        def misfit_gradient(xi, y, Gamma, solver=None):
            n = np.asarray(self.obs_index).size
            y = np.asarray(y, dtype=np.float64).reshape(n)
            Gamma = np.asarray(Gamma, dtype=np.float64).reshape(n, n)
            G, d = self._adjoint(xi, lambda G: np.linalg.solve(Gamma, G - y), solver)
            r = G - y
            return 0.5 * float(r @ np.linalg.solve(Gamma, r)), d[:, 0]

        def gradient_device(engine, U_dev, out=None):
            self.ensure_installed(engine)
            return engine.darcy_grad(U_dev, out=out)

        self.jacobian = jacobian
        self.misfit_gradient = misfit_gradient
        self.gradient_device = gradient_device
        return self

    def _device_scatter(self):
        """The Nmesh^2 slot of the KL array each parameter lands on (``eval_rf``'s reshape: the identity)."""
        return np.arange(int(self.p))

    def device_descriptor(self, n_obs=None):
        """What cesx_darcy_set takes (include/cesx.h), computed once in fp64 with this module's own calls:
        ``coef`` (K, K) with the factor K folded in and the constant mode zeroed (gaussrnd_coarse), ``D`` with
        ``idctn(L) == D @ L @ D.T``, ``S`` / ``R`` with ``_interp2_spline(centres, z, nodes) == S @ z @ S.T`` and
        ``_interp2_spline(nodes, P, centres) == R @ P @ R.T``, ``scatter`` and ``obs_index``.
        ``ValueError`` where only the host map ``model(xi)`` applies."""
        host = "; evaluate the map on the host (model(xi), enka.G_ens) instead"
        if getattr(self, "obs_index", None) is None:
            raise ValueError("darcy forward_device: obs_index is not set" + host)
        K = int(self.Nmesh)
        if K != self.Nmesh or K < self.DEVICE_NMESH[0]:
            raise ValueError("darcy forward_device: Nmesh = %r < 4 (or not an integer)" % (self.Nmesh,) + host)
        streamed = self.device_solver == "streamed"
        if streamed and K > self.DEVICE_NMESH_STREAMED[1]:
            raise ValueError("darcy forward_device: Nmesh = %d > %d is not supported on the device (streamed solver)"
                             % (K, self.DEVICE_NMESH_STREAMED[1]) + host)
        if not streamed and K > self.DEVICE_NMESH[1]:
            raise ValueError("darcy forward_device: Nmesh = %d > 16 is not supported on the device" % K + host
                             + " (or set_device_solver('streamed'), Nmesh up to %d)" % self.DEVICE_NMESH_STREAMED[1])
        obs = np.asarray(self.obs_index).reshape(-1)
        if n_obs is not None and obs.size != int(n_obs):
            raise ValueError("darcy forward_device: len(obs_index) = %d differs from the engine's n_obs = %d" % (obs.size, n_obs)
                             + host)
        scatter = np.asarray(self._device_scatter()).reshape(-1)
        if obs.size and (obs.min() < 0 or obs.max() >= K * K):
            raise ValueError("darcy forward_device: obs_index out of range" + host)
        k = np.arange(K)
        K1, K2 = np.meshgrid(k, k)
        coef = K * (self.tau ** (self.alpha - 1) * (np.pi ** 2 * (K1 ** 2 + K2 ** 2) + self.tau ** 2) ** (-self.alpha / 2))
        coef[0, 0] = 0.0
        eye = np.eye(K)
        centres = np.arange(1, 2 * K, 2) / (2.0 * K)
        nodes = np.linspace(0.0, 1.0, K)
        desc = dict(K=K, coef=coef, scatter=scatter.astype(np.int32), D=idctn(eye, axes=[0], norm="ortho"),
                    S=CubicSpline(centres, eye, axis=0, bc_type="not-a-knot", extrapolate=True)(nodes),
                    R=CubicSpline(nodes, eye, axis=0, bc_type="not-a-knot", extrapolate=True)(centres),
                    obs_index=obs.astype(np.int32))
        if streamed:
            desc.update(solver="streamed", max_workgroups=int(self.device_max_workgroups))
        return desc

    def _fingerprint(self):
        rank = getattr(self, "rank", None)
        return (float(self.alpha), float(self.tau), float(self.Nmesh), int(self.p),
                None if rank is None else np.asarray(rank).tobytes(),
                None if getattr(self, "obs_index", None) is None else np.asarray(self.obs_index).tobytes(),
                self.device_solver, int(self.device_max_workgroups))

    def invalidate_device(self):
        """Forget the map installed in an engine: the next ``forward_device`` builds and installs the descriptor again."""
        self._dev_fp = None
        self._dev_token = 0

    def ensure_installed(self, engine):
        """Make THIS map the Darcy map installed in ``engine``: installed once, again when alpha, tau, Nmesh, p, rank,
        obs_index, the device solver or its grid bound changed or another model installed its map on the same engine (``invalidate_device()`` forces it)."""
        fp = self._fingerprint()
        if (getattr(self, "_dev_fp", None) != fp
                or getattr(engine, "_darcy_token", None) is not getattr(self, "_dev_token", 0)):
            desc = self.device_descriptor(engine.n_obs)
            if desc["scatter"].size != engine.p:
                raise ValueError("darcy forward_device: the model's p = %d differs from the engine's p = %d"
                                 % (desc["scatter"].size, engine.p))
            self._dev_token = engine.darcy_set(desc)
            self._dev_fp = fp

    def forward_device(self, engine, U_dev, out=None):
        """G (n_obs, J) = this map of the columns of the device tensor ``U_dev`` (p, J), on the device.
        ``numpy.linalg.LinAlgError`` names the first particle whose system is exactly singular."""
        self.ensure_installed(engine)
        return engine.darcy_apply(U_dev, out=out)


class model_trunc(model):
    """Rank-ordered truncated KL expansion (ces/darcy.py:100-138)."""

    def __init__(self, alpha=2., tau=3., Nmesh=2. ** 4, p=10):
        super().__init__(alpha=alpha, tau=tau, Nmesh=Nmesh)
        super().set_rank()
        self.p = p

    def set_initial(self, seed=1):
        np.random.seed(seed)
        ustar = np.random.normal(0, 1, int(self.Nmesh * self.Nmesh))
        self.ustar = ustar[self.rank[:self.p]]

    def eval_rf(self, xi):
        full = np.zeros(int(self.Nmesh * self.Nmesh))
        full[self.rank[:self.p]] = np.copy(xi)
        return gaussrnd_coarse(full.reshape(int(self.Nmesh), -1), self.alpha, self.tau, self.Nmesh)

    def _device_scatter(self):
        return np.asarray(self.rank[:self.p])
