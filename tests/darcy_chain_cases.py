"""Shared cases of the Darcy chain tests (tests/test_darcy_chain_host.py, tests/test_gpu_darcy_chain.py): the Langevin and leapfrog
entry points under ``cesx_mh_grad_source(CESX_MH_GRAD_READY)`` (include/cesx.h; ces_amd/csrc/kernels_darcy_chain.hip).

Written from the header's formulas, not from ``ces_amd.sample``: with G [n][M] and d = d phi_d / du [p][M] handed over ready-made,

    phi      = 1/2 (G - y)^T Gamma^{-1} (G - y) + 1/2 (u - mu)^T Sigma^{-1} (u - mu)
    grad phi = d + Sigma^{-1} (u - mu),      g = S^T grad phi
    begin    r = xi - (e / 2) g(U),  Q = U + e S r          leap    r = r - e g(Q),  Q = Q + e S r
    accept   r = r - (e / 2) g(Q);  margin = phi(U) - phi(Q) + (|xi|^2 / 2 - |r|^2 / 2);  log u < margin accepts
    alpha    = min(1, exp(margin)), 0 for a NaN

(e = 1 unless the handle is armed; the Langevin step is begin + accept.)  The problem and the yardsticks of the whole step are
darcy_grad_cases' (``step_problem``, ``host_score``, ``np_step``): imported, not edited.

The stage bound.  A stage test holds ONE launch to fp64 from what it read: the device's own G and d go into the restatement
below, and |dev - ref| <= c eps B entry by entry, eps = 2^-52, B the same expression in absolute values, c the number of
roundings the longest chain of the expression passes through.  With u = eps / 2 the unit roundoff, a sum of m products
accumulated in ANY order (fused or not) is within m u sum |a_i b_i| to first order; the device and the numpy reference each
make such an error, so m eps covers the two.  Counting m per quantity (n = n_obs, p the dimension):

    w = L v (a triangular row, + the subtraction that formed v or follows it)     m + 1 on |L| |v|,  m = n or p
    s (the chain of n + p fused adds over squares of such rows)                   n + p adds, twice the row's m + 1 from the
                                                                                  square, the final halving exact:
                                                                                  C_PHI = 3 (n + p) + 4 on B_phi
    prior[q] = (L^T w)[q] (dense) or sw[q] (x - mu)[q]                            <= 2 p + 1 on |L|^T |L| (|x| + |mu|)
    grad phi[q] = prior[q] + d[q]                                                 one add:  2 p + 2 on B_prior + |d|
    g[r] = sum_{q >= r} S[q][r] grad phi[q]                                       p more:   C_G = 3 p + 2 on B_g = |S|^T (B_prior + |d|)
    Q = U + e S (xi - (e / 2) g)                                                  p for the row of S, 3 for the kick, the scaling
                                                                                  and the add:  C_Q = C_G + p + 4 on
                                                                                  B_Q = |U| + e |S| (|xi| + (e / 2) B_g)
    Q' = Q + e S (r - e g(Q))                                                     the same count on B_Q' = |Q| + e |S| (B_r + e B_g(Q)),
                                                                                  B_r = |xi| + (e / 2) B_g(U) carried along
    margin                                                                        the two phi, and the norms of p squares of r:
                                                                                  C_M = 2 C_PHI + 2 (C_G + p + 4) on
                                                                                  B_m = B_phi(U) + B_phi(Q) + |xi|^2 / 2 + B_r_end^2
An fp32 engine stores U and Q rounded to fp32: 2^-24 |value| on top, where a value is stored.
These are worst cases of the sum lengths, not fitted numbers: the measured ratios are a small fraction of 1 (NOTEBOOK.md).

So that "what the kernel read" is known exactly, the dense Gamma and the dense prior of the stage tests have Cholesky factors
with exact inverses: L = 2^k (I + a sub-diagonal of +-1/2), whose inverse has the entries +-2^-(i-j) / 2^k -- the host
factorisation of cesx_set_problem (a Cholesky, a triangular inverse) makes no rounding error on them, and y is rounded so
that L^{-1} y is exact as well (checked on the CPU in tests/test_darcy_chain_host.py).
"""
import functools

import numpy as np

import darcy_cases as dc
import darcy_grad_cases as gc

EPS = 2.0 ** -52
STAGE_SHAPES = [(8, 10, 12, 130), (4, 1, 3, 1), (16, 70, 5, 3), (16, 256, 4, 2)]      # (K, p, n_obs, M)
# delta of the injected single step (L = 1 and L = 3) and of the model_mh runs: the step of the host leapfrog chain of
# tests/test_darcy_grad_host.py.  np_step accepts 87 to 106 of the 130 chains there; at 0.3, the host Langevin chain's step, 129 or 130
STEP_DELTA = 1.8
MARGIN_MIN = 1e-6
SEEDS = {("diag", 1): 11, ("diag", 3): 12, ("dense", 1): 13, ("dense", 3): 14}        # (checked on the CPU: every |margin| > MARGIN_MIN)


def c_phi(n, p):
    return 3 * (n + p) + 4


def c_g(p):
    return 3 * p + 2


def c_q(p):
    return c_g(p) + p + 4


def c_m(n, p):
    return 2 * c_phi(n, p) + 2 * c_q(p)


def exact_factor(m, k):
    """(L, L^{-1}) with L = 2^k (I + a sub-diagonal of alternating +-1/2): both exact in fp64, and so is L L^T."""
    L = np.eye(m)
    for i in range(1, m):
        L[i, i - 1] = 0.5 if i % 2 else -0.5
    Li = np.eye(m)
    for i in range(m):
        for j in range(i - 1, -1, -1):
            Li[i, j] = -L[j + 1, j] * Li[i, j + 1]
    s = 2.0 ** k
    return s * L, Li / s


def make_model(K, p, n_obs):
    from ces_amd import darcy
    if K == 4:                                            # (dc.make_model's shapes start at K = 5; p = 1: the truncated expansion)
        mdl = darcy.model_trunc(Nmesh=4.0, p=p) if p < 16 else darcy.model(Nmesh=4.0)
        mdl.obs_index = np.array([5, 10, 3])[:n_obs]
        mdl.n_obs = n_obs
        return mdl.enable_gradient()
    return gc.make_model(K, p, n_obs)


@functools.lru_cache(maxsize=None)
def stage_problem(K, p, n, M, gkind, pkind, dtype):
    """The problem of one stage case: the model, y, Gamma, the prior, the scale S, the start states and the injected blocks, every
    input rounded to the engine dtype where the engine holds it in that dtype, and the factors the engine forms from them."""
    mdl = make_model(K, p, n)
    rng = np.random.default_rng(9000 + 100 * K + p + n)
    truth = 0.5 * rng.standard_normal(p)
    g0 = np.asarray(mdl(truth), dtype=np.float64)
    gs = float(np.max(np.abs(g0)))
    kG = int(np.round(np.log2(0.05 * gs)))
    y = g0 + 2.0 ** kG * rng.standard_normal(n)
    y = np.round(y * 2.0 ** (20 - kG)) * 2.0 ** (kG - 20)                  # multiples of 2^(kG - 20): L^{-1} y is exact
    if gkind == "diag":
        Gam = np.diag((2.0 ** kG * (1.0 + np.arange(n) / n)) ** 2)
        f = dict(gw=1.0 / np.diag(Gam), Lg=None, yw=y)
    else:
        L, Li = exact_factor(n, kG)
        Gam = L @ L.T
        f = dict(gw=np.ones(n), Lg=Li, yw=Li @ y)
    mu = 0.1 * rng.standard_normal(p)
    if pkind == "diag":
        cov = np.diag(1.0 + np.arange(p) / p)
        f.update(sw=1.0 / np.diag(cov), LSi=None)
    else:
        L, Li = exact_factor(p, 0)
        cov = L @ L.T
        f.update(sw=None, LSi=Li)
    f.update(mu=mu, n=n, p=p)
    S = np.tril(rng.standard_normal((p, p))) / np.sqrt(p) + np.eye(p)
    S *= 0.2
    rnd = lambda a: a.astype(dtype).astype(np.float64)    # noqa: E731
    U0 = rnd(truth[:, None] + 0.3 * rng.standard_normal((p, M)))
    xi = rnd(rng.standard_normal((3, p, M)))
    out = dict(model=mdl, y=y, Gamma=Gam, mean=mu, cov=cov, S=S, U0=U0, xi=xi, f=f)
    for v in list(out.values()) + list(f.values()):
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def factors(prob):
    """What cesx_set_problem forms from a problem of darcy_grad_cases (any SPD Gamma and cov): 1 / Gamma_ii or L_Gamma^{-1} and the
    whitened y, 1 / Sigma_ii or L_Sigma^{-1}."""
    Gam, cov = np.asarray(prob["Gamma"]), np.asarray(prob["cov"])
    n, p = Gam.shape[0], cov.shape[0]
    f = dict(mu=np.asarray(prob["mean"], dtype=np.float64), n=n, p=p)
    if np.all(Gam == np.diag(np.diag(Gam))):
        f.update(gw=1.0 / np.diag(Gam), Lg=None, yw=np.asarray(prob["y"]))
    else:
        Li = np.linalg.inv(np.linalg.cholesky(Gam))
        f.update(gw=np.ones(n), Lg=Li, yw=Li @ prob["y"])
    if np.all(cov == np.diag(np.diag(cov))):
        f.update(sw=1.0 / np.diag(cov), LSi=None)
    else:
        f.update(sw=None, LSi=np.linalg.inv(np.linalg.cholesky(cov)))
    return f


def ready_score(f, S, X, G, d):
    """phi, g = S^T grad phi and their absolute-value companions B_phi, B_g of the columns of X (p, M) from G (n, M) and d (p, M)."""
    yw = f["yw"][:, None]
    if f["Lg"] is None:
        r = G - yw
        s = np.sum(f["gw"][:, None] * r * r, axis=0)
        Bs = np.sum(f["gw"][:, None] * (np.abs(G) + np.abs(yw)) ** 2, axis=0)
    else:
        r = f["Lg"] @ G - yw
        s = np.sum(r * r, axis=0)
        Bs = np.sum((np.abs(f["Lg"]) @ np.abs(G) + np.abs(yw)) ** 2, axis=0)
    mu = f["mu"][:, None]
    dx, ax = X - mu, np.abs(X) + np.abs(mu)
    if f["LSi"] is None:
        sw = f["sw"][:, None]
        s = s + np.sum(sw * dx * dx, axis=0)
        prior, Bp = sw * dx, sw * ax
        Bs = Bs + np.sum(sw * ax * ax, axis=0)
    else:
        w, W = f["LSi"] @ dx, np.abs(f["LSi"]) @ ax
        s = s + np.sum(w * w, axis=0)
        prior, Bp = f["LSi"].T @ w, np.abs(f["LSi"]).T @ W
        Bs = Bs + np.sum(W * W, axis=0)
    return dict(phi=0.5 * s, g=S.T @ (prior + d), Bphi=0.5 * Bs, Bg=np.abs(S).T @ (Bp + np.abs(d)))


def ready_begin(S, U, xi, sU, e=1.0):
    """(Q, r, B_Q, B_r) of the first position from the score sU of the states."""
    r = xi - 0.5 * e * sU["g"]
    Br = np.abs(xi) + 0.5 * e * sU["Bg"]
    return U + e * (S @ r), r, np.abs(U) + e * (np.abs(S) @ Br), Br


def ready_leap(S, Q, r, Br, sQ, e=1.0):
    """(Q', r', B_Q', B_r') of the full kick at Q and the next position; a non-finite phi(Q) poisons r[0]."""
    r2 = r - e * sQ["g"]
    r2[0, ~np.isfinite(sQ["phi"])] = np.nan
    Br2 = Br + e * sQ["Bg"]
    return Q + e * (S @ r2), r2, np.abs(Q) + e * (np.abs(S) @ Br2), Br2


def ready_margin(sU, sQ, xi, r, Br, e=1.0):
    """(margin without log u, B_m) of the test at the last position Q."""
    re = r - 0.5 * e * sQ["g"]
    Bre = Br + 0.5 * e * sQ["Bg"]
    m = sU["phi"] - sQ["phi"] + (0.5 * np.sum(xi * xi, axis=0) - 0.5 * np.sum(re * re, axis=0))
    return m, sU["Bphi"] + sQ["Bphi"] + 0.5 * np.sum(xi * xi, axis=0) + np.sum(Bre * Bre, axis=0)


def alpha_of(margin):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.where(margin >= 0, 1.0, np.where(margin < 0, np.exp(np.minimum(margin, 0.0)), 0.0))


def host_grad(prob, X):
    """(G, d) of the columns of X on the host: the model's own adjoint, one solve per column."""
    mdl, y, Gam = prob["model"], np.asarray(prob["y"]), np.asarray(prob["Gamma"])
    G, d = np.empty((y.size, X.shape[1])), np.empty(X.shape)
    for j in range(X.shape[1]):
        Gj, dj = mdl._adjoint(X[:, j], lambda g: np.linalg.solve(Gam, g - y))
        G[:, j], d[:, j] = Gj, dj[:, 0]
    return G, d


def ready_step(prob, f, S, U, xi, logu, L, grad=None):
    """One Langevin (L = 1) / leapfrog step of every column of U through the READY formulas: (Q, accept mask, margin - log u,
    U_next), the tuple of gc.np_step.  ``grad(X)`` returns (G, d); the host adjoint by default."""
    grad = (lambda X: host_grad(prob, X)) if grad is None else grad
    sU = ready_score(f, S, U, *grad(U))
    Q, r, _, Br = ready_begin(S, U, xi, sU)
    for _ in range(L - 1):
        Q, r, _, Br = ready_leap(S, Q, r, Br, ready_score(f, S, Q, *grad(Q)))
    m, _ = ready_margin(sU, ready_score(f, S, Q, *grad(Q)), xi, r, Br)
    acc = m - logu > 0
    return Q, acc, m - logu, np.where(acc[None, :], Q, U)


# ---- the end-to-end step on darcy_grad_cases.step_problem: M_STEP chains from Ustar, injected blocks ----

def step_scale(prob, delta):
    return delta * np.linalg.cholesky(np.cov(prob["Ustar"]))


def injected(gkind, L, dtype="float64"):
    """The xi (p, M) and log u (M,) blocks the GPU tests inject into the single step, from the seed of the case."""
    K, p, n = gc.STEP_SHAPE
    rng = np.random.default_rng(SEEDS[(gkind, L)])
    xi = rng.standard_normal((p, gc.M_STEP)).astype(dtype).astype(np.float64)
    return xi, np.log(rng.uniform(size=gc.M_STEP))


@functools.lru_cache(maxsize=None)
def step_reference(gkind, L, dtype="float64"):
    """gc.np_step on the injected blocks, and per chain the bound of Q: at every position X of the numpy trajectory the adjoint
    bound b(X) = 16 cond_2(A) 2^-52 s(X) of darcy_grad_cases.bound on every entry of d, carried to first order through
    Q_L = U + S (L xi - (L - 1/2) g(U) - sum_k (L - k) g(Q_k)),  g = S^T (d + prior):  |S| |S|^T 1 (L - 1/2) b(U) + ... ."""
    prob = gc.step_problem(gkind)
    S = step_scale(prob, STEP_DELTA)
    U = np.array(prob["Ustar"]).astype(dtype).astype(np.float64)
    xi, logu = injected(gkind, L, dtype)
    Q, acc, margin, Un = gc.np_step(prob, S, U, xi, logu, L)
    mdl, y, Gi = prob["model"], np.asarray(prob["y"]), np.abs(np.linalg.inv(prob["Gamma"]))
    SS1 = (np.abs(S) @ np.abs(S).T) @ np.ones(S.shape[0])

    def b(x):
        cond = np.linalg.cond(gc.operator_matrix(mdl, x))
        assert cond < dc.COND_MAX
        return 16.0 * cond * gc.EPS * np.max(np.abs(mdl.jacobian(x)).T @ (Gi @ (np.abs(mdl(x)) + np.abs(y))))
    bound = np.empty((S.shape[0], gc.M_STEP))
    for j in range(gc.M_STEP):
        w = (L - 0.5) * b(U[:, j])
        r = xi[:, j] - 0.5 * gc.host_score(prob, S, U[:, j])[1]
        q = U[:, j] + S @ r
        for k in range(1, L):
            w += (L - k) * b(q)
            r = r - gc.host_score(prob, S, q)[1]
            q = q + S @ r
        bound[:, j] = SS1 * w
    out = dict(prob=prob, S=S, U=U, xi=xi, logu=logu, Q=Q, acc=acc, margin=margin, U_next=Un, bound=bound)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out
