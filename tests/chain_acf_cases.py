"""Shared cases of the tests of the streaming lagged sums (tests/test_chain_acf_host.py, tests/test_gpu_chain_acf.py;
cesx_chain_acf_*, kernels_chainacf.hip): the shapes, the synthetic traces, the extended-precision numpy reference of every
output of cesx_chain_acf_read, the estimator written out from its definition, and the error bounds.  Everything here runs on
the host.

The bounds.  u = 2^-53; a floating-point sum of K terms added in order errs by at most (K - 1) u sum|terms| to first order.
Every bound is  c 2^-52 B  = 2 c u B with B the summed expression with every term replaced by its absolute value: the kernel's
own roundings take at most half of it (c counts them), the other half is left to the reference (extended precision: far less).
With a_t = x_t - x_0 (one rounding each), A1 = sum|a_t| and d = S1 / N:

  chain_gamma   G_k = P_k - d (Hd_k + Tl_k) + (N - k) d^2.
                P_k: N - k products a_t a_{t+k} (two rounded factors: 2 u) added by one fma each (N - k roundings): (N + 2) u sum|a_t a_{t+k}|.
                S1: N terms of one rounding each, N - 1 additions: N u A1; d = S1 / N one more: |delta d| <= (N + 1) u A1 / N.
                Hd_k and Tl_k: k additions of the window, one subtraction, on |values| <= A1: (k + 1) u A1 each, on top of S1's
                N u A1; their sum and the product with d: 2 more.  |Hd_k + Tl_k| <= 2 A1, so
                |delta (d (Hd_k + Tl_k))| <= [(N + 1) + (N + k + 3)] u |d| 2 A1 <= (2 N + L + 4) u (2 |d| A1) with |d| A1 >= N d^2.
                (N - k) d^2: 2 (N + 1) u |d| A1 (N - k) / N + 3 u (N - k) d^2, inside (2 N + 4) u [(N - k) d^2 + 2 |d| A1] with the line above.
                The two final additions: 2 u B.  Altogether <= (2 N + L + 8) u B_k <= (N + L + 8) 2^-52 B_k with
                B_k = sum|a_t a_{t+k}| + 2 |d| A1 + (N - k) d^2:     c_chain = N + L + 8.
  chain_mean    m = x_0 + d: (N + 1) u A1 / N + u |m|:  c = N + 4 over B = |x_0| + A1 / N.
  pooled sums   chain_acf_reduce_kernel: a thread adds every 256th chain in order (ceil(C / 256) terms), then a tree of 8
                levels over the threads, a division and the store: depth c_red = ceil(C / 256) + 8 + 2.
                gsum_k: the terms' own errors plus the reduce over |G_k| <= B_k:  (c_chain + c_red) 2^-52 sum_j B_k.
                cbar = mean of the first draws (device: the same reduce, then / C): |delta cbar| <= c_red 2^-52 mean|x_0|.
                msum = sum (m_j - cbar): sum_j delta m_j + C delta cbar + c_red 2^-52 sum|m_j - cbar| (the reference subtracts
                its own, exact, cbar).  m2sum = sum (m_j - cbar)^2: sum_j [2 |m_j - cbar| e_j + e_j^2] + c_red 2^-52 m2sum
                with e_j = delta m_j + delta cbar + 2^-52 |m_j - cbar|.
"""
import functools

import numpy as np

EPS = 2.0 ** -52
LAGS_MAX = 64                    # CESX_CHAIN_ACF_LAGS_MAX
BLOCK, RT = 64, 256              # kernels_chainacf.hip: ACF_BLOCK, ACF_RT
LD = np.longdouble


def lt_of(L):
    """The ring's slots (acf_lt of kernels_chainacf.hip): 8 and 32 run on registers, 64 on the LDS ring."""
    return 8 if L <= 8 else (32 if L <= 32 else 64)


def n_set(L):
    """The issue's N in {L + 2, 2 L - 1, 3 L + 5}, each lifted to the stage's minimum max(4, L + 2)."""
    lo = max(4, L + 2)
    return sorted({lo, max(lo, 2 * L - 1), 3 * L + 5})


# (p, J, C, L, N): a pairwise selection over p in {1, 3, 65}, J in {1, 63, 65, 257}, C in {J - 1, 1} (C = J where J = 1),
# L in {1, 2, 31, 64} and the N of ``n_set``, and L = 8 | 9 and 32 | 33 where ``lt_of`` changes the kernel.  N > 64 goes
# through the in-place path when added at once, everything else through the stage's pending block.
CASES = (
    (1, 1, 1, 1, 4), (65, 257, 1, 1, 8), (3, 63, 62, 1, 4),
    (3, 63, 62, 2, 4), (3, 65, 64, 2, 11), (65, 65, 1, 2, 4),
    (3, 257, 256, 31, 33), (1, 257, 1, 31, 61), (65, 63, 62, 31, 98), (1, 65, 64, 31, 98),
    (3, 65, 64, 64, 66), (1, 63, 62, 64, 127), (3, 257, 256, 64, 197), (65, 65, 1, 64, 66),
    (1, 65, 64, 8, 29), (3, 63, 1, 9, 32), (3, 65, 64, 32, 101), (1, 65, 1, 33, 104),
)


def chunkings(N, L):
    """How the N draws are cut into add calls: at once, one at a time, the issue's uneven pieces (1, L - 1, L, L + 1, rest)
    and a short piece ahead of the rest (the pending block filled up by a long add, the remainder read in place)."""
    uneven, left = [], N
    for k in (1, L - 1, L, L + 1):
        k = min(k, left)
        if k > 0:
            uneven.append(k)
            left -= k
    if left:
        uneven.append(left)
    out = {"one": [N], "singles": [1] * N, "uneven": uneven}
    if N > 5:
        out["head5"] = [5, N - 5]
    return out


def make_trace(p, J, N, dtype, seed=0):
    """(N, p, J) draws as the engine holds them (rounded to the engine dtype), in fp64: AR(1) chains of different scales per
    row about chain-specific offsets; chain 1 (J > 1) sits at 10^6 x its spread; chain 2 (J > 2) is stuck for the whole run."""
    rng = np.random.default_rng([seed, p, J, N])
    e = rng.standard_normal((N, p, J))
    x = np.empty((N, p, J))
    x[0] = e[0]
    for t in range(1, N):
        x[t] = 0.7 * x[t - 1] + np.sqrt(1 - 0.49) * e[t]
    x = x * (10.0 ** rng.uniform(-2, 2, p))[None, :, None] + 0.5 * rng.standard_normal((1, p, J))
    if J > 1:
        x[:, :, 1] = 1e6 * (1 + np.arange(p))[None, :] + e[:, :, 1]
    if J > 2:
        x[:, :, 2] = x[0:1, :, 2]
    return x.astype(dtype).astype(np.float64)


MUTANTS = ("draw_dropped", "lag_off_by_one", "no_head_tail", "history_not_carried", "sums_about_zero")


def ref_raw(trace, C, L, mutant=None, form="centred", boundary=None):
    """Every output of cesx_chain_acf_read for the draws ``trace`` (N, p, J), its first C chains and lags 0 .. L, in numpy's
    extended precision (rounded to fp64 at the end), with B of every output under ``B_<name>``.
    ``form``: 'centred' -- sum (x_t - m)(x_{t+k} - m) with the chain's mean m, the definition -- or 'shifted' -- the device's
    P_k - d (Hd_k + Tl_k) + (N - k) d^2 about the first draw.  ``mutant``: one of MUTANTS -- the reference made wrong on
    purpose (``boundary``: the add boundary the history is lost at), for the host test that the bounds see it."""
    x = np.asarray(trace, dtype=np.float64)[:, :, :C].astype(LD)
    if mutant == "draw_dropped":
        x = x[:-1]
    N, p, _ = x.shape
    c = x[0]
    a = x - c[None]
    A1 = np.abs(a).sum(axis=0)
    S1 = a.sum(axis=0)
    d = S1 / N
    m = c + d
    if mutant == "sums_about_zero":                        # no shift: fp64 sums of x_t x_{t+k}, as a kernel would form them
        xf = np.asarray(x, dtype=np.float64)
        s1 = np.zeros((p, C))
        for t in range(N):
            s1 = s1 + xf[t]
        df = s1 / N
    gamma, B = np.empty((L + 1, p, C), dtype=LD), np.empty((L + 1, p, C), dtype=LD)
    for k in range(L + 1):
        kk = min(k + 1, N - 1) if (mutant == "lag_off_by_one" and k > 0) else k
        B[k] = (np.abs(a[:N - k]) * np.abs(a[k:])).sum(axis=0) + 2 * np.abs(d) * A1 + (N - k) * d * d
        if mutant == "sums_about_zero":
            P = np.zeros((p, C))
            for t in range(k, N):
                P = P + xf[t - k] * xf[t]
            hd, tl = s1 - xf[N - k:].sum(axis=0), s1 - xf[:k].sum(axis=0)
            gamma[k] = (P - df * (hd + tl) + (N - k) * df * df).astype(LD)
        elif form == "shifted" or mutant in ("no_head_tail", "history_not_carried"):
            prod = a[:N - kk] * a[kk:]                       # term i: a_i a_{i+k}, added at t = i + k
            if mutant == "history_not_carried":
                t = np.arange(kk, N)
                prod = prod[~((t - kk < boundary) & (t >= boundary))]
            P = prod.sum(axis=0)
            hd, tl = S1 - a[N - kk:].sum(axis=0), S1 - a[:kk].sum(axis=0)
            if mutant == "no_head_tail":
                hd, tl = S1, S1
            gamma[k] = P - d * (hd + tl) + (N - kk) * d * d
        else:
            z = a - d[None]                                # x_t - m with m = x_0 + d: a_t is exact in extended precision
            gamma[k] = (z[:N - kk] * z[kk:]).sum(axis=0)
    cbar = c.sum(axis=1) / C
    dm = m - cbar[:, None]
    f = lambda v: np.asarray(v, dtype=np.float64)          # noqa: E731
    return dict(N=N, C=C, L=L, chain_gamma=f(gamma), chain_mean=f(m), gsum=f(gamma.sum(axis=2).T), msum=f(dm.sum(axis=1)),
                m2sum=f((dm * dm).sum(axis=1)), B_chain_gamma=f(B), B_chain_mean=f(np.abs(c) + A1 / N),
                B_cbar=f(np.abs(c).sum(axis=1) / C), dm_abs=f(np.abs(dm)))


def c_chain(N, L):
    return N + L + 8


def c_red(C):
    return -(-C // RT) + 8 + 2


def raw_bounds(ref):
    """{output: elementwise bound} of cesx_chain_acf_read against ``ref_raw`` (the derivation: the module's docstring)."""
    N, C, L = ref["N"], ref["C"], ref["L"]
    cc, cr = c_chain(N, L) * EPS, c_red(C) * EPS
    d_gamma = cc * ref["B_chain_gamma"]
    d_mean = (N + 4) * EPS * ref["B_chain_mean"]
    d_cbar = cr * ref["B_cbar"]
    e = d_mean + d_cbar[:, None] + EPS * ref["dm_abs"]
    return dict(chain_gamma=d_gamma, chain_mean=d_mean,
                gsum=(d_gamma.sum(axis=2) + cr * ref["B_chain_gamma"].sum(axis=2)).T,
                msum=d_mean.sum(axis=1) + C * d_cbar + cr * ref["dm_abs"].sum(axis=1),
                m2sum=(2 * ref["dm_abs"] * e + e * e).sum(axis=1) + cr * (ref["dm_abs"] ** 2).sum(axis=1))


def ratio(got, ref, bound):
    """max |got - ref| / bound; an entry whose bound is 0 must be met exactly."""
    err = np.abs(np.asarray(got) - ref)
    zero = bound == 0
    assert np.all(err[zero] == 0), "an entry with a zero bound differs"
    return float(np.max(err[~zero] / bound[~zero])) if np.any(~zero) else 0.0


@functools.lru_cache(maxsize=None)
def case_ref(case, dtype):
    """(trace, reference, bounds) of one of CASES in an engine dtype: computed once, shared, never written to."""
    p, J, C, L, N = case
    x = make_trace(p, J, N, dtype)
    ref = ref_raw(x, C, L)
    x.setflags(write=False)
    return x, ref, raw_bounds(ref)


def estimator_ref(raw, n, M_total, C, L):
    """The autocorrelation ESS from raw sums, written out from its definition, independently of
    ces_amd.sample.finalise_autocorr: (rho (p, L + 1), tau, ess, truncated, W, var+)."""
    g = np.asarray(raw["gsum"], dtype=np.float64)
    p = g.shape[0]
    rho, tau, ess = np.full((p, L + 1), np.nan), np.full(p, np.nan), np.full(p, np.nan)
    trunc, Ws, vps = np.zeros(p, dtype=bool), np.zeros(p), np.zeros(p)
    for r in range(p):
        W = g[r, 0] / (C * (n - 1))
        Bn = (raw["m2sum"][r] - raw["msum"][r] ** 2 / C) / (C - 1) if C > 1 else 0.0
        vp = (n - 1) / n * W + max(Bn, 0.0)
        Ws[r], vps[r] = W, vp
        if not vp > 0:
            continue
        rho[r] = [1.0] + [1 - (W - g[r, k] / (C * n)) / vp for k in range(1, L + 1)]
        pairs = [rho[r, 2 * t] + rho[r, 2 * t + 1] for t in range((L + 1) // 2)]
        neg = [i for i, v in enumerate(pairs) if v < 0]
        trunc[r] = not neg
        pairs = pairs[:neg[0]] if neg else pairs
        mono = [min(pairs[:i + 1]) for i in range(len(pairs))]
        tau[r] = -1 + 2 * sum(mono)
        ess[r] = M_total * n / tau[r]
    return rho, tau, ess, trunc, Ws, vps


def ar1(phi, p, n, M, rng):
    """(p, n, M) AR(1) chains x_t = phi x_{t-1} + eps, eps ~ N(0, 1), from the stationary law."""
    x = np.empty((p, n, M))
    x[:, 0] = rng.standard_normal((p, M)) / np.sqrt(1 - phi * phi)
    for t in range(1, n):
        x[:, t] = phi * x[:, t - 1] + rng.standard_normal((p, M))
    return x
