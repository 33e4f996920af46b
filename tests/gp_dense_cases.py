"""Case tables, the numpy reference and the bar of the dense per-chain likelihood (CESX_GP_DENSE, kernels_gpdense.hip):
    d = B m_j + g0 - y,   Sigma_j = Gamma + B diag(v_j) B^T,
    phi_j = 1/2 d^T Sigma_j^{-1} d [+ 1/2 log det Sigma_j] + 1/2 (x_j - mu)^T Sigma_prior^{-1} (x_j - mu).
Shared by tests/test_gp_dense_host.py and tests/test_gpu_gp_dense.py; imports without a device.

The reference is the literal form of ces/sample.py:52-57, :69-72: ``np.linalg.solve(2 Sigma, d)``,
``1/2 sum log eigvals(Sigma)`` and the prior's ``logpdf`` without its constant (the quadratic form, through
``np.linalg.solve``), evaluated at the states as the engine dtype rounds them.

The bar, per chain j, with q_j = 1/2 d^T Sigma_j^{-1} d and eps = 2^-52:
    bound_j = 16 eps (n + cond_2(Sigma_j)) (q_j + [logdet]) + (p + 8) eps (the prior term in absolute values).
The constant 16 comes from the reference's own error, measured without the code under test (``measure_reference_error``
below restates that measurement): over 14 shapes, n in {1, 2, 7, 50, 63, 64, 65, 96, 128}, v in [1e-8, 1], cond_2(Sigma) up
to 2.8e8, 24 chains each, against an 80-bit long-double Cholesky taken as the truth, a fixed-order fp64 Cholesky and the
LU-based reference form both stay within 1.64 cond_2 eps q (worst at n = 1; <= 0.9 for n >= 2); the log det by Cholesky
within 2.6e4 n eps absolute (< 1e-3 of (n + cond_2) eps), the reference's eigvals form within 0.4 n eps cond_2.  16 is
about 10 x the worst measured ratio, the reference's own error included.  Score inputs keep cond_2(Sigma_j) <= 1e8, the
accept-loop inputs <= 1e6 (asserted where the cases are built)."""
import numpy as np

from oracle import stage_ref as sr

EPS = 2.0 ** -52
NMAX = 128
COND_SCORE, COND_ACCEPT = 1e8, 1e6

# (n, k, cond_2(Gamma), kind): 'pca' a B with orthogonal columns of mixed scales, 'cmp' B = I (the dense compounded likelihood)
HOST_CASES = [(1, 1, 1, "pca"), (2, 1, 10, "pca"), (7, 3, 1e2, "pca"), (50, 8, 1e4, "pca"), (63, 16, 1e4, "pca"),
              (64, 64, 1e4, "pca"), (65, 5, 1e4, "pca"), (96, 12, 1e4, "pca"), (128, 16, 1e4, "pca"), (128, 128, 1e4, "pca"),
              (2, 2, 10, "cmp"), (50, 50, 1e4, "cmp"), (65, 65, 1e4, "cmp"), (128, 128, 1e4, "cmp")]
HOST_M = 24
# the shapes of the measurement behind the constant 16 (cond_2(Sigma) up to 2.8e8: two of them lie past the test inputs' 1e8)
MEASURE_CASES = [(n, k, 1e6 if (n, k) in ((96, 12), (128, 128)) else c, kind) for n, k, c, kind in HOST_CASES]
FAMILIES = ("pca", "cmp")

GPU_N = [1, 2, 63, 64, 65, 127, 128]
GPU_SHAPES = [(n, k) for n in GPU_N for k in sorted({1, 3, n}) if k <= n]
GPU_M = [1, 5, 257]


def problem(rng, n, k, cond_gamma, kind, p=3, dense_prior=False, b_scale=(-2.0, 1.0)):
    """Gamma, B, g0, y of one case and a prior (mu, Sigma_prior) of dimension p."""
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    ev = np.exp(np.linspace(0.0, -np.log(cond_gamma), n)) if n > 1 else np.ones(1)
    Gam = 0.01 * (Q * ev) @ Q.T
    Gam = (Gam + Gam.T) / 2
    if kind == "pca":
        B = np.linalg.qr(rng.standard_normal((n, k)))[0] * np.exp(rng.uniform(b_scale[0], b_scale[1], k))
    else:
        assert k == n
        B = np.eye(n)
    g0 = rng.standard_normal(n)
    y = g0 + 0.1 * rng.standard_normal(n)
    mu = 0.1 * rng.standard_normal(p)
    if dense_prior:
        Bs = rng.standard_normal((p, p)) / np.sqrt(p)
        Sp = 0.5 * (Bs @ Bs.T) + 0.5 * np.eye(p)
    else:
        Sp = np.diag(0.5 + rng.random(p))
    return dict(n=n, k=k, p=p, Gamma=Gam, B=np.ascontiguousarray(B), g0=g0, y=y, mu=mu, Sp=Sp)


def rows(rng, k, M, v_lo=1e-8):
    """Crafted GP rows (k, M): means of the size of the data misfit, variances log-uniform in [v_lo, 1]."""
    return 0.3 * rng.standard_normal((k, M)), np.exp(rng.uniform(np.log(v_lo), 0.0, (k, M)))


def states(rng, pr, M, dtype=np.float64):
    return (pr["mu"][:, None] + 0.5 * rng.standard_normal((pr["p"], M))).astype(dtype)


def sigma_of(pr, v):
    return pr["Gamma"] + (pr["B"] * v) @ pr["B"].T


def prior_term(pr, X):
    """1/2 (x - mu)^T Sigma_prior^{-1} (x - mu) per column, and the same sum with every term in absolute value."""
    e = np.asarray(X, dtype=np.float64) - pr["mu"][:, None]
    Si = np.linalg.inv(pr["Sp"])
    return 0.5 * (e * np.linalg.solve(pr["Sp"], e)).sum(axis=0), 0.5 * (np.abs(e) * (np.abs(Si) @ np.abs(e))).sum(axis=0)


def reference(pr, m, v, X, logdet):
    """(phi, bound, cond_2, q) per chain: the literal form and its bar.  A chain whose Sigma is not positive definite
    (a non-positive eigenvalue) has phi = NaN and bound = NaN."""
    n, p, M = pr["n"], pr["p"], m.shape[1]
    pt, pt_abs = prior_term(pr, X)
    phi, bound, cond, qs = np.empty(M), np.empty(M), np.empty(M), np.empty(M)
    for j in range(M):
        Sig = sigma_of(pr, v[:, j])
        d = pr["B"] @ m[:, j] + pr["g0"] - pr["y"]
        ev = np.linalg.eigvalsh(Sig)                       # (ascending; cond_2 of a symmetric positive definite matrix)
        if not ev[0] > 0.0:
            phi[j] = bound[j] = cond[j] = qs[j] = np.nan
            continue
        q = (d * np.linalg.solve(2 * Sig, d)).sum()
        ph = q + pt[j]
        if logdet:
            ph += 0.5 * np.log(np.linalg.eigvals(Sig)).sum().real
        cond[j] = ev[-1] / ev[0]
        qs[j] = q
        phi[j] = ph
        bound[j] = 16 * EPS * (n + cond[j]) * (q + (1.0 if logdet else 0.0)) + (p + 8) * EPS * pt_abs[j]
    return phi, bound, cond, qs


def kernel_order(pr, m, v, X, logdet, mutant=None):
    """phi per chain in the order of gp_score_dense_kernel, all chains at once: column c of Sigma from
    Gamma_ic + sum_t B_it (v_t B_ct) (t increasing), the left-looking update over the earlier columns in increasing order,
    the pivot, the division of the column; the forward substitution z_c = d_c / L_cc, d_i -= L_ic z_c; z_c^2 and log L_cc
    summed in column order; then the prior term as gp_score_kernel forms it (w = L_prior^{-1} (x - mu) for a dense
    prior).  A pivot that is not > 0 or not finite: NaN.  (numpy rounds the product and the sum where the kernel fuses
    them.)  mutant: one of MUTANTS -- a deliberately wrong kernel, for the test of the bar's teeth."""
    n, k, p, M = pr["n"], pr["k"], pr["p"], m.shape[1]
    B, Gam, g0 = pr["B"], pr["Gamma"], pr["g0"]
    kk = k - 1 if mutant == "last_column" else k
    d = np.zeros((M, n))
    for t in range(k):
        d += B[:, t][None, :] * m[t][:, None]
    if mutant != "g0":
        d = d + g0[None, :]
    d = d - pr["y"][None, :]
    L = np.zeros((M, n, n))
    q, ld, bad = np.zeros(M), np.zeros(M), np.zeros(M, dtype=bool)
    nsub = n - 1 if mutant == "last_row" else n
    with np.errstate(invalid="ignore", divide="ignore"):
        for c in range(n):
            s = np.zeros((M, n - c))
            for t in range(kk):
                if mutant == "diagonal":
                    s[:, 0] += B[c, t] * (v[t] * B[c, t])
                else:
                    s += B[c:, t][None, :] * (v[t] * B[c, t])[:, None]
            if mutant != "gamma":
                s = Gam[c, c:][None, :] + s
            for cc in range(c):
                s -= L[:, c:, cc] * L[:, c, cc][:, None]
            piv = s[:, 0]
            bad |= ~((piv > 0.0) & np.isfinite(piv))
            l = np.sqrt(piv)
            col = s / l[:, None]
            col[:, 0] = l
            L[:, c:, c] = col
            if c < nsub:
                zc = d[:, c] / l
                q += zc * zc
                d[:, c + 1:] -= col[:, 1:] * zc[:, None]
            if logdet and mutant != "logdet":
                ld += np.log(l)
    e = np.asarray(X, dtype=np.float64) - pr["mu"][:, None]
    Sp = pr["Sp"]
    if np.any(Sp != np.diag(np.diag(Sp))):
        Li = np.linalg.inv(np.linalg.cholesky(Sp))
        sp = np.zeros(M)
        for r in range(p):
            w = np.zeros(M)
            for t in range(r + 1):
                w += Li[r, t] * e[t]
            sp += w * w
    else:
        sp = np.zeros(M)
        for r in range(p):
            sp += (1.0 / Sp[r, r]) * (e[r] * e[r])
    with np.errstate(invalid="ignore"):
        ph = 0.5 * q + ld + 0.5 * sp
    return np.where(bad, np.nan, ph)


def mutant_is_identity(mutant, n, k, kind, logdet):
    """The cases on which a mutant computes the same function: no log det term to drop; B diag(v) B^T is its own diagonal
    for B = I and for n = 1."""
    return (mutant == "logdet" and not logdet) or (mutant == "diagonal" and (kind == "cmp" or n == 1))


# deliberately wrong kernels: each must leave 4 x bound on some chain of every case of every family it can show in
MUTANTS = ("logdet",        # the log det term dropped
           "gamma",         # Gamma dropped from Sigma
           "diagonal",      # only the diagonal of B diag(v) B^T kept
           "last_column",   # the last column of B ignored in Sigma
           "g0",            # g0 dropped from d
           "last_row")      # row n - 1 left out of the substitution


def measure_reference_error(cases=MEASURE_CASES, M=HOST_M):
    """The measurement behind the constant 16, restated: worst ratios, over the cases, of (a) a fixed-order fp64 Cholesky
    and (b) the LU-based reference form to cond_2 eps q for the quadratic term, (c) the Cholesky log det to n eps and (d)
    the eigvals log det to n eps cond_2, each against an 80-bit long-double Cholesky.  No code under test is involved."""
    def chol(S, d, dt):
        n = len(d)
        S, d = S.astype(dt), d.astype(dt)
        L = np.zeros((n, n), dtype=dt)
        for c in range(n):
            L[c, c] = np.sqrt(S[c, c] - np.dot(L[c, :c], L[c, :c]))
            for i in range(c + 1, n):
                L[i, c] = (S[i, c] - np.dot(L[i, :c], L[c, :c])) / L[c, c]
        z = np.zeros(n, dtype=dt)
        for i in range(n):
            z[i] = (d[i] - np.dot(L[i, :i], z[:i])) / L[i, i]
        return dt(0.5) * np.dot(z, z), np.log(np.diag(L)).sum()
    worst = np.zeros(4)
    for n, k, cg, kind in cases:
        rng = np.random.default_rng([n, k, int(cg), kind == "pca"])
        pr = problem(rng, n, k, cg, kind)
        m, v = rows(rng, k, M)
        for j in range(M):
            Sig = sigma_of(pr, v[:, j])
            d = pr["B"] @ m[:, j] + pr["g0"] - pr["y"]
            cond = np.linalg.cond(Sig)
            qt, lt = (float(x) for x in chol(Sig, d, np.longdouble))
            qc, lc = chol(Sig, d, np.float64)
            qr = (d * np.linalg.solve(2 * Sig, d)).sum()
            lr = 0.5 * np.log(np.linalg.eigvals(Sig)).sum().real
            worst = np.maximum(worst, [abs(qc - qt) / (cond * EPS * abs(qt)), abs(qr - qt) / (cond * EPS * abs(qt)),
                                       abs(lc - lt) / (n * EPS), abs(lr - lt) / (n * EPS * cond)])
    return worst


class DenseAcceptRef(sr.AcceptRef):
    """oracle.stage_ref.AcceptRef with the band of the dense mode: half-width max(1e-9 max(1, |phi|), bound(U) + bound(P)),
    the bound of every chain's current state carried along with its phi.  ``half_width(bound_p)`` is called once per
    step, before ``decide``; ``commit`` then moves the bounds of the chains that took their proposal."""

    def __init__(self, phi0, bound0):
        super().__init__(phi0)
        self.bound = np.array(bound0, dtype=np.float64)
        self.bound_p = None

    def half_width(self, bound_p):
        self.bound_p = np.asarray(bound_p, dtype=np.float64)
        with np.errstate(invalid="ignore"):
            return np.maximum(sr.BAND * np.maximum(1.0, np.abs(self.phi)), self.bound + self.bound_p)

    def commit(self, taken, phi_p, band=None):
        super().commit(taken, phi_p, band)
        self.bound = np.where(np.asarray(taken, dtype=bool), self.bound_p, self.bound)
