"""Shared cases of the streamed Darcy device-map tests (tests/test_gpu_darcy_stream.py, tests/test_darcy_stream_host.py).

The conventions are ``darcy_cases.reference``'s exactly: the yardstick is the host map ``ces_amd.darcy.model.__call__`` in
fp64, particle by particle; the seed is 300000 + 1000 K + 10 p + scale; the draw is (p, 130) and a case takes its leading
columns; the inputs are rounded to the engine dtype before the host evaluates them; the bound is ``darcy_cases.tolerance``.
Each reference is computed once per (shape, scale, input dtype), only for the particles the shape's tests use, and shared.

For K >= 48 cond_2(A) comes from ``eigvalsh`` of the symmetric A, max|lambda| / min|lambda| (the singular values of a
symmetric matrix are the moduli of its eigenvalues); the dense SVD of ``darcy_cases.host_parts`` is far slower there.
"""
import functools

import numpy as np

import darcy_cases as dc

# (K, p, n_obs) -> the particles its tests use
SHAPES = {(4, 16, 3): 32,          # n = 4 is smaller than the window: the ring never wraps
          (16, 256, 50): 32,       # the resident kernel's largest shape (a case of darcy_cases.SHAPES)
          (17, 20, 9): 32,         # the first mesh past the resident limit, model_trunc
          (18, 324, 11): 32,       # full model, p = K^2
          (33, 1089, 50): 8,       # odd m = 31, full model
          (64, 64, 50): 2}         # the LDS limit, the largest workspace slot
SCALES = dc.SCALES
COND_MAX = dc.COND_MAX
EIGVALSH_FROM = 48
SHAPE_IDS = ["K%d-p%d-n%d" % s for s in SHAPES]


def make_model(K, p, n_obs, solver="streamed"):
    mdl = dc.make_model(K, p, n_obs)
    if solver is not None:
        mdl.set_device_solver(solver)
    return mdl


def host_parts(mdl, xi):
    """(g, cond_2(A), min nodal coefficient) of one particle on the host path; as ``darcy_cases.host_parts``, cond_2 from the
    eigenvalues once the mesh is large."""
    from ces_amd import darcy
    K = int(mdl.Nmesh)
    if K < EIGVALSH_FROM:
        return dc.host_parts(mdl, xi)
    theta = mdl.eval_rf(xi)
    centres = np.arange(1, 2 * K, 2) / (2.0 * K)
    nodes = np.linspace(0.0, 1.0, K)
    a = darcy._interp2_spline(centres, np.exp(theta), nodes)
    A = darcy.assemble_gwf(a).toarray()
    assert np.array_equal(A, A.T)
    lam = np.abs(np.linalg.eigvalsh(A))
    return mdl(xi), lam.max() / lam.min(), a.min()


def host(mdl, U):
    parts = [host_parts(mdl, U[:, j]) for j in range(U.shape[1])]
    return dict(G=np.stack([q[0] for q in parts], axis=1), cond=np.array([q[1] for q in parts]),
                amin=np.array([q[2] for q in parts]))


@functools.lru_cache(maxsize=None)
def reference(K, p, n_obs, scale, dtype):
    """The leading ``SHAPES[(K, p, n_obs)]`` columns of ``darcy_cases.reference``'s draw and their host values."""
    J = SHAPES[(K, p, n_obs)]
    if (K, p, n_obs) in dc.SHAPES:
        full = dc.reference(K, p, n_obs, scale, dtype)
        out = dict(model=full["model"], U=full["U"][:, :J], G=full["G"][:, :J], cond=full["cond"][:J], amin=full["amin"][:J])
        return out
    mdl = dc.make_model(K, p, n_obs)
    rng = np.random.default_rng(300000 + 1000 * K + 10 * p + scale)
    U = (scale * rng.standard_normal((p, dc.JMAX))).astype(dtype).astype(np.float64)[:, :J].copy()
    out = dict(model=mdl, U=U, **host(mdl, U))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def check(G, ref, dtype, case, worst=None):
    """Every particle of G (n_obs, J) within ``darcy_cases.tolerance`` of the host reference.  Returns the largest
    err / (cond_2(A) 2^-52 max|g_host|) of the case (the bound is 16 of these units, plus the output rounding for fp32)."""
    J = G.shape[1]
    tol, gmax, cond = dc.tolerance(ref, dtype, J)
    err = np.max(np.abs(G - ref["G"][:, :J]), axis=0)
    ratio = float(np.max(err / (cond * 2.0 ** -52 * gmax)))
    if worst is not None and np.dtype(dtype) == np.float64 and ratio > worst["ratio"]:
        worst.update(ratio=ratio, case=case)
    bad = np.nonzero(~(err <= tol))[0]
    assert bad.size == 0, (case, "particles", bad[:5], "err", err[bad[:5]], "bound", tol[bad[:5]], "cond", cond[bad[:5]])
    return ratio
