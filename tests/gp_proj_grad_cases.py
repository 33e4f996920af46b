"""Case tables, the bars and the numpy restatement of the gradient coefficients of the projected per-chain likelihood
(gp_proj_coef_kernel, kernels_gpprojgrad.hip; include/cesx.h, cesx_gp_proj_coef):
    phi_data = 1/2 d^T Sigma^{-1} d [+ 1/2 log det Sigma],   d = B m + g0 - y,   Sigma = Gamma + B diag(v) B^T,
    e_t = B_t^T Sigma^{-1} d,   h_t = B_t^T Sigma^{-1} B_t,   a_t = e_t,   b_t = 1/2 ([logdet] h_t - e_t^2).
Shared by tests/test_gp_proj_grad_host.py and tests/test_gpu_gp_proj_langevin.py; imports without a device.  The problems, rows
and shapes are those of tests/gp_dense_cases.py (gc) and tests/gp_proj_cases.py (gq).

The reference is the literal n-space form (``literal``): ``np.linalg.solve`` with Sigma_j per chain.  The bars, per chain and
t, with cond = max(cond_2(Sigma_j), cond_2(Gamma)), q = 1/2 d^T Sigma^{-1} d and eps = 2^-52:
    |e_t - ref| <= C_E eps (n + cond) sqrt(2 q h_t)          (|e_t| <= sqrt(2 q h_t) by Cauchy-Schwarz in the Sigma^{-1} product)
    |h_t - ref| <= C_H eps (n + cond) h_t
    |b_t - ref| <= 1/2 ([logdet] bar_h + 2 |e_t| bar_e + bar_e^2)                                  (propagated from both)
    |phi_data - ref| <= 16 eps (n + cond) (q + [logdet])     (gp_proj_cases.reference's bar without its prior term)

The constants come from the reference's own error, measured without the code under test (``measure_reference_error`` below,
over MEASURE_CASES = gq.HOST_SHAPES and gq.BIG_B, 8 chains each, v in [1e-8, 1]): against an 80-bit long-double Cholesky in
n-space taken as the truth, the worst ratios to eps (n + cond) sqrt(2 q h_t) resp. eps (n + cond) h_t are
    e: the literal fp64 form (solve)   0.45        a fixed-order fp64 Cholesky   0.61
    h: the literal fp64 form (solve)   0.30        a fixed-order fp64 Cholesky   0.90
(all four worst at n = 1, where n + cond = 2; <= 0.1 for n >= 7).  About 10 x the worst ratio of each, rounded up to a power
of two: C_E = 8, C_H = 16.  The reference's own error is part of that margin.
Coefficient inputs keep cond_2(Sigma_j) <= gc.COND_SCORE, accept-loop inputs <= gc.COND_ACCEPT (asserted where the cases are
built)."""
import functools

import numpy as np

import gp_dense_cases as gc
import gp_proj_cases as gq

EPS = gc.EPS
C_E, C_H = 8.0, 16.0

# (n, k, cond_2(Gamma), b_scale)
MEASURE_CASES = [(n, k, gq.cond_gamma_of(n), (-2.0, 1.0)) for n, k in gq.HOST_SHAPES] + [(gq.BIG_B[0], gq.BIG_B[1], 1e4, gq.BIG_B[2])]
MEASURE_M = 8


def literal(pr, m, v, logdet):
    """The literal n-space form per chain: dict of phi (the data term), e, h (k, M), q, cond = max(cond_2(Sigma_j),
    cond_2(Gamma)) and cond_s = cond_2(Sigma_j) alone.  The log det is 1/2 sum log eigvalsh(Sigma_j) (Sigma is symmetric; the
    eigenvalues are needed for cond_2 anyway).  NaN where Sigma_j is not positive definite."""
    n, k, M = pr["n"], pr["k"], m.shape[1]
    B = pr["B"]
    gam = np.linalg.eigvalsh(pr["Gamma"])
    cond_g = gam[-1] / gam[0]
    out = dict(phi=np.full(M, np.nan), q=np.full(M, np.nan), cond=np.full(M, np.nan), cond_s=np.full(M, np.nan),
               e=np.full((k, M), np.nan), h=np.full((k, M), np.nan))
    for j in range(M):
        Sig = gc.sigma_of(pr, v[:, j])
        ev = np.linalg.eigvalsh(Sig)
        if not ev[0] > 0.0:
            continue
        d = B @ m[:, j] + pr["g0"] - pr["y"]
        sol = np.linalg.solve(Sig, np.column_stack([d, B]))
        q = 0.5 * (d * sol[:, 0]).sum()
        out["q"][j] = q
        out["phi"][j] = q + (0.5 * np.log(ev).sum() if logdet else 0.0)
        out["cond_s"][j] = ev[-1] / ev[0]
        out["cond"][j] = max(ev[-1] / ev[0], cond_g)
        out["e"][:, j] = B.T @ sol[:, 0]
        out["h"][:, j] = (B * sol[:, 1:]).sum(axis=0)
    return out


def coef_b(e, h, logdet):
    return 0.5 * ((h if logdet else 0.0) - e * e)


def bars(pr, ref, logdet):
    """(bar_phi (M,), bar_e, bar_h, bar_b (k, M)) of the module docstring from ``literal``'s dict."""
    scale = EPS * (pr["n"] + ref["cond"])
    bar_e = C_E * scale * np.sqrt(2.0 * ref["q"] * ref["h"])
    bar_h = C_H * scale * ref["h"]
    bar_b = 0.5 * ((bar_h if logdet else 0.0) + 2.0 * np.abs(ref["e"]) * bar_e + bar_e * bar_e)
    return 16 * scale * (ref["q"] + (1.0 if logdet else 0.0)), bar_e, bar_h, bar_b


@functools.lru_cache(maxsize=None)
def coef_case(n, k, M, cond_gamma=1e4, b_scale=(-2.0, 1.0), seed=0, cond_cap=gc.COND_SCORE, v_lo=1e-8):
    """One problem with M crafted chains and its literal reference (log det included in phi_ld, absent from phi_q), built
    once per shape and shared: (pr, m, v, ref).  The arrays are read-only."""
    rng = np.random.default_rng([n, k, M, seed, 77])
    pr = gc.problem(rng, n, k, cond_gamma, "pca", b_scale=b_scale)
    m, v = gc.rows(rng, k, M, v_lo=v_lo)
    ref = literal(pr, m, v, True)
    assert cond_cap is None or np.all(ref["cond_s"] <= cond_cap), ref["cond_s"].max()
    ref["phi_ld"], ref["phi_q"] = ref.pop("phi"), ref["q"]
    for a in (m, v) + tuple(ref.values()):
        a.setflags(write=False)
    return pr, m, v, ref


def take(ref, logdet, cols=None):
    """``literal``'s dict for one log det value (and a subset of ``coef_case``'s chains)."""
    c = slice(None) if cols is None else cols
    out = {key: ref[key][..., c] for key in ("q", "cond", "cond_s", "e", "h")}
    out["phi"] = (ref["phi_ld"] if logdet else ref["phi_q"])[c]
    return out


def kernel_order_proj_coef(pr, m, v, logdet, mutant=None, proj=None):
    """(phi_data (M,), a (k, M), b (k, M)) in the order of gp_proj_coef_kernel, all chains at once: the factor and the
    forward substitution of gp_proj_cases.kernel_order_proj (z kept); the back substitution w_c = z_c / L_cc, z_i -= L_ci w_c
    for c = k - 1 .. 0; e_t = sum_i R_it w_i, i increasing; X = L^{-1} by columns right to left, X_ij = -(sum_{s = j + 1 .. i}
    X_is L_sj) / L_jj, s increasing; h_t = sum_i (sum_{s <= min(i, t)} X_is R_st)^2; b = 1/2 ([logdet] h - e^2).  (numpy rounds
    the product and the sum where the kernel fuses them.)  A pivot that is not > 0 or not finite: NaN in all three.
    mutant: one of MUTANTS."""
    k, M = pr["k"], m.shape[1]
    R, a0, c_perp, hld = gq.project(pr) if proj is None else proj
    R = np.triu(R)
    a = np.zeros((M, k))
    for t in range(k):
        a += R[:, t][None, :] * m[t][:, None]
    a = a + a0[None, :]
    L = np.zeros((M, k, k))
    z = np.zeros((M, k))
    q = np.full(M, c_perp)
    ld = np.full(M, hld if logdet else 0.0)
    bad = np.zeros(M, dtype=bool)
    with np.errstate(invalid="ignore", divide="ignore"):
        for c in range(k):
            s = np.zeros((M, k - c))
            for t in range(c, k):
                s += R[c:, t][None, :] * (v[t] * R[c, t])[:, None]
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
            z[:, c] = zc
            q += zc * zc
            a[:, c + 1:] -= col[:, 1:] * zc[:, None]
            if logdet:
                ld += np.log(l)
        w = np.zeros((M, k))
        if mutant == "w_is_z":                    # no back substitution
            w = z.copy()
        else:
            zz = z.copy()
            for c in range(k - 1, -1, -1):
                w[:, c] = zz[:, c] / L[:, c, c]
                zz[:, :c] -= L[:, c, :c] * w[:, c][:, None]
        e = np.zeros((M, k))
        kk = k - 1 if mutant == "e_last_column" else k          # R's last column ignored in e
        for i in range(k):
            e[:, :kk] += R[i, :kk][None, :] * w[:, i][:, None]
        if mutant == "e_sign":
            e = -e
        h = np.zeros((M, k))
        if logdet and mutant != "no_h":
            X = np.zeros((M, k, k))
            for j in range(k - 1, -1, -1):
                acc = np.zeros((M, k - j - 1))
                for s_ in range(j + 1, k):
                    acc[:, s_ - j - 1:] += X[:, s_:, s_] * L[:, s_, j][:, None]
                X[:, j + 1:, j] = -acc / L[:, j, j][:, None]
                X[:, j, j] = 1.0 / L[:, j, j]
            for i in range(k):
                y = np.zeros((M, k))
                top = i if mutant == "h_short" else i + 1       # the inner sum of h stops before the diagonal entry X_ii
                for s_ in range(top):
                    y += X[:, i, s_][:, None] * R[s_][None, :]
                h += y * y
        b = 0.5 * (h - e * e)
        ph = 0.5 * q + ld
    nan = np.where(bad, np.nan, 0.0)
    return ph + nan, (e + nan[:, None]).T, (b + nan[:, None]).T


# deliberately wrong kernels: each must leave 4 x the bar, in a or in b, on some chain of every case where it is not the identity
MUTANTS = ("w_is_z",           # w taken as z: no back substitution
           "no_h",             # the h term dropped from b
           "e_sign",           # e's sign flipped
           "e_last_column",    # R's last column ignored in e
           "h_short")          # the inner sum of h without its diagonal entry


def mutant_is_identity(mutant, logdet):
    """Without the log det flag there is no h term to drop or to shorten."""
    return mutant in ("no_h", "h_short") and not logdet


def measure_reference_error(cases=MEASURE_CASES, M=MEASURE_M):
    """The measurement behind C_E and C_H, restated: worst ratios, over the cases, of the literal fp64 form (solve) and of a
    fixed-order fp64 Cholesky form to eps (n + cond) sqrt(2 q h_t) for e and to eps (n + cond) h_t for h, each against an
    80-bit long-double Cholesky in n-space: [e literal, e Cholesky, h literal, h Cholesky].  No code under test is involved."""
    def chol_form(Sig, rhs, dt):
        n = Sig.shape[0]
        S, Y = Sig.astype(dt), rhs.astype(dt)
        L = np.zeros((n, n), dtype=dt)
        for c in range(n):
            L[c, c] = np.sqrt(S[c, c] - np.dot(L[c, :c], L[c, :c]))
            if c + 1 < n:
                L[c + 1:, c] = (S[c + 1:, c] - L[c + 1:, :c] @ L[c, :c]) / L[c, c]
        for i in range(n):                                       # Y := L^{-1} [d | B]
            Y[i] = (Y[i] - L[i, :i] @ Y[:i]) / L[i, i]
        return Y[:, 1:].T @ Y[:, 0], (Y[:, 1:] * Y[:, 1:]).sum(axis=0), dt(0.5) * np.dot(Y[:, 0], Y[:, 0])
    worst = np.zeros(4)
    for n, k, cg, b_scale in cases:
        rng = np.random.default_rng([n, k, int(cg), 5])
        pr = gc.problem(rng, n, k, cg, "pca", b_scale=b_scale)
        m, v = gc.rows(rng, k, M)
        ref = literal(pr, m, v, False)
        for j in range(M):
            Sig = gc.sigma_of(pr, v[:, j])
            d = pr["B"] @ m[:, j] + pr["g0"] - pr["y"]
            rhs = np.column_stack([d, pr["B"]])
            et, ht, qt = (np.asarray(x, dtype=np.float64) for x in chol_form(Sig, rhs, np.longdouble))
            ec, hc, _ = chol_form(Sig, rhs, np.float64)
            scale = EPS * (n + ref["cond"][j])
            be, bh = scale * np.sqrt(2.0 * qt * ht), scale * ht
            worst = np.maximum(worst, [np.max(np.abs(ref["e"][:, j] - et) / be), np.max(np.abs(ec - et) / be),
                                       np.max(np.abs(ref["h"][:, j] - ht) / bh), np.max(np.abs(hc - ht) / bh)])
    return worst
