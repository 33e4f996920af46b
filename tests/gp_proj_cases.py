"""Case tables, the bar and the numpy restatement of the projected per-chain likelihood (CESX_GP_PROJ, kernels_gpproj.hip):
the likelihood of tests/gp_dense_cases.py with Sigma_j = Gamma + B diag(v_j) B^T projected to k x k
(ces_amd.emulate.project_sigma).  Shared by tests/test_gp_proj_host.py and tests/test_gpu_gp_proj.py; imports without a device.

The reference is ``gp_dense_cases.reference``: the literal ``solve(2 Sigma, d)`` / ``eigvals`` form.  The bar is that
module's bound_j with cond_2(Sigma_j) replaced by max(cond_2(Sigma_j), cond_2(Gamma)):
    bound_j = 16 eps (n + max(cond_2(Sigma_j), cond_2(Gamma))) (q_j + [logdet]) + (p + 8) eps (the prior term in absolute values).
The host reduction solves with Gamma alone (L_Gamma^{-1} B, L_Gamma^{-1} (g0 - y)), so Gamma's conditioning enters whatever
v is.  The constant stays 16: its measurement is ``gp_dense_cases.measure_reference_error``, which involves no code under
test."""
import numpy as np

import gp_dense_cases as gc

EPS = gc.EPS
KMAX = 128

# (n, k): n_obs past the dense mode's 128, k at and around the group widths 16 / 32 / 64 and the two-slot range
HOST_SHAPES = [(1, 1), (7, 3), (50, 8), (128, 16), (129, 4), (180, 16), (180, 128), (300, 64), (65, 65)]
# ... and the regime B diag(v) B^T >> Gamma (b_scale = (2, 5): columns of B of norm e^2 .. e^5), where a Woodbury form cancels
BIG_B = (180, 16, (2.0, 5.0))
HOST_M = gc.HOST_M

GPU_K = [1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128]
GPU_SHAPES = [(max(k, 129), k) for k in GPU_K] + [(180, 16), (300, 64)]
GPU_M = gc.GPU_M


def cond_gamma_of(n):
    return 1 if n == 1 else 1e2 if n < 50 else 1e4


def reference(pr, m, v, X, logdet):
    """(phi, bound, cond, q) per chain: gp_dense_cases.reference with the projected mode's bar, cond = max(cond_2(Sigma_j),
    cond_2(Gamma)); the fifth value is cond_2(Sigma_j) alone.  NaN where Sigma_j is not positive definite."""
    phi, _, cond_s, q = gc.reference(pr, m, v, X, logdet)
    ev = np.linalg.eigvalsh(pr["Gamma"])
    cond = np.maximum(cond_s, ev[-1] / ev[0])
    _, pt_abs = gc.prior_term(pr, X)
    bound = 16 * EPS * (pr["n"] + cond) * (q + (1.0 if logdet else 0.0)) + (pr["p"] + 8) * EPS * pt_abs
    return phi, bound, cond, q, cond_s


def project(pr):
    from ces_amd import emulate
    return emulate.project_sigma(pr["Gamma"], pr["B"], pr["g0"], pr["y"])


def kernel_order_proj(pr, m, v, X, logdet, mutant=None, proj=None):
    """phi per chain in the order of gp_score_proj_kernel, all chains at once: a = (sum_t R_it m_t, t increasing) + a0;
    column c of A = I + R diag(v) R^T from sum_{t >= c} R_it (v_t R_ct) (t increasing; R's zeros below the diagonal add
    nothing), 1 added to the diagonal entry, the left-looking update over the earlier columns in increasing order, the
    pivot, the division of the column; the forward substitution z_c = a_c / L_cc, a_i -= L_ic z_c; q = c_perp + sum z_c^2
    and half_logdet_gamma + sum log L_cc in column order; then the prior term as gp_score_kernel forms it.  A pivot that is
    not > 0 or not finite: NaN.  (numpy rounds the product and the sum where the kernel fuses them.)  mutant: one of
    MUTANTS -- a deliberately wrong kernel, for the test of the bar's teeth."""
    k, p, M = pr["k"], pr["p"], m.shape[1]
    R, a0, c_perp, hld = project(pr) if proj is None else proj
    kk = k - 1 if mutant == "last_column" else k
    a = np.zeros((M, k))
    for t in range(k):
        a += R[:, t][None, :] * m[t][:, None]
    if mutant != "a0":
        a = a + a0[None, :]
    L = np.zeros((M, k, k))
    q = np.full(M, 0.0 if mutant == "c_perp" else c_perp)
    ld = np.full(M, hld if logdet and mutant != "half_logdet_gamma" else 0.0)
    bad = np.zeros(M, dtype=bool)
    with np.errstate(invalid="ignore", divide="ignore"):
        for c in range(k):
            s = np.zeros((M, k - c))
            for t in range(c, kk):
                s += R[c:, t][None, :] * (v[t] * R[c, t])[:, None]
            if mutant != "identity":
                s[:, 0] = 1.0 + s[:, 0]
            for cc in range(c):
                s -= L[:, c:, cc] * L[:, c, cc][:, None]
            piv = s[:, 0]
            bad |= ~((piv > 0.0) & np.isfinite(piv))
            l = np.sqrt(piv)
            col = s / l[:, None]
            col[:, 0] = l
            L[:, c:, c] = col
            zc = a[:, c] / l
            q += zc * zc
            a[:, c + 1:] -= col[:, 1:] * zc[:, None]
            if logdet:
                ld += np.log(l)
    e = np.asarray(X, dtype=np.float64) - pr["mu"][:, None]
    Sp = pr["Sp"]
    sp = np.zeros(M)
    if np.any(Sp != np.diag(np.diag(Sp))):
        Li = np.linalg.inv(np.linalg.cholesky(Sp))
        for r in range(p):
            w = np.zeros(M)
            for t in range(r + 1):
                w += Li[r, t] * e[t]
            sp += w * w
    else:
        for r in range(p):
            sp += (1.0 / Sp[r, r]) * (e[r] * e[r])
    with np.errstate(invalid="ignore"):
        ph = 0.5 * q + ld + 0.5 * sp
    return np.where(bad, np.nan, ph)


# deliberately wrong kernels: each must leave 4 x bound on some chain of every case where it is not the identity
MUTANTS = ("c_perp",              # c_perp dropped from the quadratic form
           "half_logdet_gamma",   # Gamma's half of the log det dropped
           "a0",                  # a0 dropped from a
           "last_column",         # the last column of R ignored in S
           "identity")            # the I of I + S dropped


def mutant_is_identity(mutant, n, k, logdet):
    """No log det term to drop; for n == k the columns of Q span everything: r_perp = 0 and c_perp is rounding."""
    return (mutant == "half_logdet_gamma" and not logdet) or (mutant == "c_perp" and n == k)
