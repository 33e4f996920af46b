"""fp64 references of the Sample and Emulate stages' device steps.

TEST INFRASTRUCTURE (see oracle/__init__.py).  Plain numpy restatements of what mh_accept_kernel and gp_score_kernel
compute from the arrays they are given, of the uniform both draw for a chain, and of the proposal a U + b S xi with the
device's noise block (oracle/philox.py).  The references take the values the device reads (already rounded to the engine
dtype), so that what is left between the two is the order of an fp64 sum; tests/test_stage_refs_host.py holds them
against the chains of the real reference (tests/golden/mcmc.npz, gp_mcmc.npz).
"""
import numpy as np

from .philox import MASK, noise_block, philox4x32_10

BAND = 1e-9                      # the bar the project holds fp64 paths to: half-width of a tie, relative to max(1, |phi|)
MH_STEP_BIT = 1 << 31            # the Philox step word of an MH draw is step | 2^31 (include/cesx.h)


def mh_step_word(step):
    return (int(step) | MH_STEP_BIT) & 0xFFFFFFFF


def log_uniform(M, seed, step, j_offset=0):
    """log u of the chains j_offset .. j_offset + M - 1 at MH step ``step``: counter (lo(gj), hi(gj), 0xffffffff,
    step | 2^31), key (seed lo, seed hi), the 53-bit integer from the first two output words, half a unit added."""
    gj = np.arange(M, dtype=np.uint64) + np.uint64(j_offset)
    lo, hi = (gj & MASK).astype(np.uint32), (gj >> np.uint64(32)).astype(np.uint32)
    c2 = np.full(M, 0xFFFFFFFF, dtype=np.uint32)
    c3 = np.full(M, mh_step_word(step), dtype=np.uint32)
    x, y, _, _ = philox4x32_10(lo, hi, c2, c3, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    m53 = ((x.astype(np.uint64) >> np.uint64(5)) << np.uint64(26)) | (y.astype(np.uint64) >> np.uint64(6))
    return np.log((m53.astype(np.float64) + 0.5) * 2.0 ** -53)


def mh_noise(p, M, seed, step, j_offset=0, dtype=np.float32):
    """The xi block cesx_mh_propose draws on the device: the engine's noise block in the MH counter domain."""
    return noise_block(p, M, seed, mh_step_word(step), j_offset, dtype)


def propose(U, S, xi, update=None, beta=0.5):
    """P = U + S xi (random walk) or sqrt(1 - beta^2) U + sqrt(beta) S xi (pCN, ces/sample.py:199, :202)."""
    U, S, xi = (np.asarray(a, dtype=np.float64) for a in (U, S, xi))
    if update == "pCN":
        return np.sqrt(1.0 - beta ** 2) * U + np.sqrt(beta) * (S @ xi)
    return U + S @ xi


def mh_phi(G, y, gw, X=None, mu=None, sw=None):
    """phi per column: 1/2 sum_i gw_i (g_i - y_i)^2 + 1/2 sum_r sw_r (x_r - mu_r)^2.  X None: no prior rows (pCN);
    mu / sw None: 0 / 1 (the rows are w = L_Sigma^{-1} (x - mu) of a dense Sigma)."""
    G = np.asarray(G, dtype=np.float64)
    d = G - np.asarray(y, dtype=np.float64)[:, None]
    s = (np.asarray(gw, dtype=np.float64)[:, None] * d * d).sum(axis=0)
    if X is not None:
        e = np.asarray(X, dtype=np.float64)
        if mu is not None:
            e = e - np.asarray(mu, dtype=np.float64)[:, None]
        e2 = e * e
        if sw is not None:
            e2 = np.asarray(sw, dtype=np.float64)[:, None] * e2
        s = s + e2.sum(axis=0)
    return 0.5 * s


def dense_prior_rows(X, mu, Sigma):
    """w = L_Sigma^{-1} (x - mu) per column, fp64."""
    L = np.linalg.cholesky(np.asarray(Sigma, dtype=np.float64))
    return np.linalg.solve(L, np.asarray(X, dtype=np.float64) - np.asarray(mu, dtype=np.float64)[:, None])


def gp_phi(mode, mean, var, y, Gamma, X, mu, Sigma):
    """phi per column of MCMC.gp_mh from the GP rows (ces/sample.py:48-60) without the terms that are constant in u:
    'gamma'      1/2 d^T Gamma^{-1} d
    'var'        1/2 sum_i d_i^2 / v_i + log v_i
    'gamma_var'  the same with v_i = Gamma_ii + var_i (a diagonal Gamma)
    plus 1/2 (x - mu)^T Sigma^{-1} (x - mu) for RW and pCN alike.  A column with any v_i <= 0 scores +inf: the proposal
    is rejected (the device's sum is NaN there and its test fails)."""
    mean = np.asarray(mean, dtype=np.float64)
    d = mean - np.asarray(y, dtype=np.float64)[:, None]
    Gamma = np.asarray(Gamma, dtype=np.float64)
    if mode == "gamma":
        s = (d * np.linalg.solve(Gamma, d)).sum(axis=0)
        bad = np.zeros(mean.shape[1], dtype=bool)
    elif mode in ("var", "gamma_var"):
        v = np.asarray(var, dtype=np.float64)
        if mode == "gamma_var":
            v = np.diag(Gamma)[:, None] + v
        bad = np.any(~(v > 0.0), axis=0)
        vs = np.where(v > 0.0, v, 1.0)
        s = (d * d / vs + np.log(vs)).sum(axis=0)
    else:
        raise ValueError("unknown likelihood mode %r" % (mode,))
    e = np.asarray(X, dtype=np.float64) - np.asarray(mu, dtype=np.float64)[:, None]
    s = s + (e * np.linalg.solve(np.asarray(Sigma, dtype=np.float64), e)).sum(axis=0)
    return np.where(bad, np.inf, 0.5 * s)


class AcceptRef(object):
    """The accept step log u < phi(U) - phi(P) over the columns, with the tie band of the device comparisons.

    ``decide`` returns the reference's decision and which chains are within the band of a tie at this step
    (|phi(U) - phi(P) - log u| <= half-width; half-width BAND max(1, |phi(U)|) unless one is given); ``commit`` takes the
    decisions that hold (the device's own for a chain in the band) and carries phi and the counters forward, so that a
    tie costs one chain-step and not the chain."""

    def __init__(self, phi0):
        self.phi = np.array(phi0, dtype=np.float64)
        self.count = np.zeros(self.phi.shape, dtype=np.int64)
        self.left_out = 0
        self.chain_steps = 0

    def decide(self, phi_p, logu, half_width=None):
        phi_p = np.asarray(phi_p, dtype=np.float64)
        logu = np.asarray(logu, dtype=np.float64)
        with np.errstate(invalid="ignore"):
            margin = self.phi - phi_p - logu
            hw = BAND * np.maximum(1.0, np.abs(self.phi)) if half_width is None else half_width
            band = np.abs(margin) <= hw
            accept = logu < self.phi - phi_p
        return accept, band

    def commit(self, taken, phi_p, band=None):
        taken = np.asarray(taken, dtype=bool)
        self.phi = np.where(taken, phi_p, self.phi)
        self.count += taken
        self.chain_steps += taken.size
        if band is not None:
            self.left_out += int(np.count_nonzero(band))

    def within_cap(self):
        """at most 1 chain-step in 1000 left out"""
        return 1000 * self.left_out <= self.chain_steps
