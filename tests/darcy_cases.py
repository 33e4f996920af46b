"""Shared cases of the Darcy device-map tests (tests/test_gpu_darcy.py, tests/test_darcy_device_host.py).

The yardstick everywhere is the host map ``ces_amd.darcy.model.__call__`` in fp64, particle by particle; each reference
is computed once per (shape, scale, input dtype) and shared by the tests that need it.
"""
import functools

import numpy as np

SHAPES = [(5, 4, 3), (6, 36, 7), (8, 10, 12), (16, 64, 50), (16, 256, 50)]      # (K, p, n_obs)
SCALES = [1, 3, 10]
JMAX = 130
COND_MAX = 1e11            # beyond it 16 cond eps says nothing; the fixed seeds stay below (asserted where the bound is used)


def make_model(K, p, n_obs):
    """``model_trunc`` whenever p < K^2, ``model`` otherwise; obs_index a fixed random subset -- at K = 8 unsorted and
    containing the last centre K^2 - 1."""
    from ces_amd import darcy
    mdl = darcy.model_trunc(Nmesh=float(K), p=p) if p < K * K else darcy.model(Nmesh=float(K))
    rng = np.random.default_rng(100 * K + n_obs)
    obs = rng.choice(K * K, n_obs, replace=False)
    if K == 8:
        obs = obs[obs != K * K - 1]
        obs = np.concatenate([obs[:3], [K * K - 1], obs[3:]])[:n_obs]
        if np.all(np.diff(obs) > 0):
            obs[:2] = obs[1::-1]
        assert obs[3] == K * K - 1 and not np.all(np.diff(obs) > 0)
    mdl.obs_index = obs
    mdl.n_obs = n_obs
    return mdl


def host_parts(mdl, xi):
    """(g, cond_2(A), min nodal coefficient) of one particle on the host path."""
    from ces_amd import darcy
    K = int(mdl.Nmesh)
    theta = mdl.eval_rf(xi)
    centres = np.arange(1, 2 * K, 2) / (2.0 * K)
    nodes = np.linspace(0.0, 1.0, K)
    a = darcy._interp2_spline(centres, np.exp(theta), nodes)
    A = darcy.assemble_gwf(a).toarray()
    return mdl(xi), np.linalg.cond(A), a.min()


@functools.lru_cache(maxsize=None)
def reference(K, p, n_obs, scale, dtype):
    """xi = scale N(0, I) from a fixed seed (JMAX columns; a test with fewer takes the leading ones), rounded to the engine
    dtype -- the host reference of an fp32 engine is evaluated at the fp32-rounded inputs."""
    mdl = make_model(K, p, n_obs)
    rng = np.random.default_rng(300000 + 1000 * K + 10 * p + scale)      # (checked on the CPU: every case below COND_MAX)
    U = (scale * rng.standard_normal((p, JMAX))).astype(dtype).astype(np.float64)
    parts = [host_parts(mdl, U[:, j]) for j in range(JMAX)]
    out = dict(model=mdl, U=U, G=np.stack([q[0] for q in parts], axis=1), cond=np.array([q[1] for q in parts]),
               amin=np.array([q[2] for q in parts]))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def tolerance(ref, dtype, J=None):
    """Per particle: 16 cond_2(A) 2^-52 max|g_host| (+ 2^-23 max|g_host| for the output rounding of an fp32 engine)."""
    sl = slice(0, J)
    gmax = np.max(np.abs(ref["G"][:, sl]), axis=0)
    cond = ref["cond"][sl]
    assert np.all(cond < COND_MAX), "a fixed seed left the range where the bound means something"
    return (16.0 * cond * 2.0 ** -52 + (2.0 ** -23 if np.dtype(dtype) == np.float32 else 0.0)) * gmax, gmax, cond


def apply_descriptor(desc, xi):
    """The descriptor of ``model.device_descriptor`` applied in numpy, the solve by ``scipy.linalg.solve_banded`` (partial-pivot
    banded LU): what the kernel computes, restated independently of it."""
    from scipy.linalg import solve_banded
    from ces_amd import darcy
    K = desc["K"]
    m = K - 2
    Xi = np.zeros(K * K)
    Xi[desc["scatter"]] = xi
    L = desc["coef"] * Xi.reshape(K, K)
    L[0, 0] = 0.0
    a = desc["S"] @ np.exp(desc["D"] @ L @ desc["D"].T) @ desc["S"].T
    A = darcy.assemble_gwf(a).toarray()
    n = m * m
    ab = np.zeros((2 * m + 1, n))
    for c in range(n):
        lo, hi = max(0, c - m), min(n, c + m + 1)
        ab[m + lo - c:m + hi - c, c] = A[lo:hi, c]
    x = solve_banded((m, m), ab, np.ones(n))
    Rp = desc["R"][:, 1:-1]
    return (Rp @ x.reshape(m, m, order="F") @ Rp.T).flatten()[desc["obs_index"]]
