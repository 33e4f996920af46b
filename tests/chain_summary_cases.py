"""Shared cases of the streaming chain summaries' tests (tests/test_chain_summary_host.py, tests/test_gpu_chain_summary.py):
the fp64 numpy reference of the raw sums of cesx_chain_summary_read and of the finalised ``MCMC.summary`` dict, the case
tables and the bounds.  Everything here runs on the host.

The bounds.  A floating-point sum of K terms, in whatever order, errs by at most d u sum|terms| to first order, d the
largest number of roundings a term passes through (its depth in the summation tree, <= K - 1) and u = 2^-53.  Every bound
below is  c 2^-52 B  with B the summed expression with every term replaced by its absolute value and c >= the kernel's depth
plus 4 (the subtraction of the shift, the product, a division, the store): at 2^-52 = 2 u the kernel's own error takes at
most half of it, which leaves the other half to the reference (numpy's extended precision here: far less).

  per-chain half sums  S1 = sum (x - shift), S2 = sum (x - shift)^2 over the n draws of a half, one lane adding them in order:
                       c = n + 4.  The half-chain mean m = shift + S1 / n and variance s^2 = (S2 - S1^2 / n) / (n - 1) carry
                       the same c over B_m = |shift| + sum|x - shift| / n and
                       B_v = (sum (x - shift)^2 + (sum|x - shift|)^2 / n) / (n - 1): d(S1^2 / n) = 2 |S1| dS1 / n
                       <= 2 (n - 1) u (sum|x - shift|)^2 / n.
  pooled sums          sum (x - c), sum (x - c)(x - c)^T over N J terms.  The kernel adds a slab of chains (``slab_plan``: at most
                       2048, fewer where the lower triangle has few super tiles) draw by draw on the MFMA (kept x slab terms of
                       depth <= kept x slab), then the slabs in a fixed order (32 lanes take every 32nd slab, then the lanes in
                       order: never deeper than slabs), then the earlier launches' total: N slab + slabs + N over all chunkings, and never more than the N J - 1 of any order of N J terms.
                       c = min(N slab + slabs + N + 4, N J + 8).
  the pooled shift     c = mean of the first draw's row: rowsum_kernel's 256 lanes take ceil(per / 256) terms of a slice each,
                       six shuffle levels, four waves, then the slices in order and the division:
                       c = ceil(per / 256) + 6 + 4 + slices + 4, per = ceil(J / slices), slices = min(64, ceil(J / 1024)).
  W and B_m            the reduce over the 2 J half-chains: 8 terms per lane (two halves, four chains), six shuffle levels, four
                       waves, ceil(J / 1024) workgroups: c3 = 8 + 6 + 4 + ceil(J / 1024) + 4, on top of the terms' own errors
                       dm <= (n + 4) 2^-52 B_m and dv <= (n + 4) 2^-52 B_v (``wb_bounds``).
The finalised values inherit these to first order (``summary_bounds``), doubled for the second-order terms and a few
roundings of the finalising arithmetic itself.
"""
import numpy as np

EPS = 2.0 ** -52
SLAB, WGS, TC, CH = 2048, 1024, 32, 1024    # kernels_chainsum.hip: CS_SLAB, CS_WGS, CS_TC, CS_CH
SLICES, RL = 64, 32                         # CS_SLICES, CS_RL

# engine level (the issue's table): every p x J x N below runs in both dtypes, both families and the three chunkings
P_SET = (1, 3, 16, 17, 33)
J_SET = (1, 2, 63, 64, 65, 130)
N_SET = (4, 5, 9)
FAMILIES = ("centred", "offset")

# The launch plan's other regimes (``plan_of``): at every shape of the table above there is one 64 x 64 super tile, one staged
# tile per slab, at most five slabs, one slice of the row sums and one workgroup of the half reduce.  (p, J, N), the smallest
# shapes that reach each regime; tests/test_chain_summary_host.py asserts from ``plan_of`` that they do.
#   (64, 65, 5)      a full single super tile: all four waves of chain_pool_kernel, wave w with w + 1 blocks
#   (65, 130, 4)     3 pairs: one row in super tile 1, the off-diagonal tile (1, 0) with one staged row of A and all 8 of B
#   (129, 65, 5)     6 pairs: si = 2, the tiles (2, 0) and (2, 1)
#   (2, 1025, 5)     33 slabs (a second pass of the 32 reduce lanes), 2 slices, 2 workgroups of the half reduce
#   (3, 32801, 4)    slabs of 64 chains (two tiles a draw), 513 slabs, the last of 33 chains (its second tile holds one),
#                    33 slices and workgroups
#   (1, 65601, 4)    slabs of 96 chains (three tiles), 684 slabs, 64 slices -- the cap, where ceil(J / 1024) = 65 --, 65 workgroups
#   (129, 5505, 4)   off-diagonal tiles and two tiles a draw together (6 pairs, 87 slabs, the last of one chain)
# Not covered: the clamp of a slab at CS_SLAB chains (``lo > want`` in cs_slab_cols) needs J > 2^21 at p <= 64, or close to a
# gigabyte of trace at a larger p.
PLAN_SHAPES = ((64, 65, 5), (65, 130, 4), (129, 65, 5), (2, 1025, 5), (3, 32801, 4), (1, 65601, 4), (129, 5505, 4))


def chunkings(N):
    return {"one": [N], "singles": [1] * N, "split": [2, N - 2]}


def make_trace(p, J, N, family, dtype, seed=0):
    """(N, p, J) draws as the engine holds them (rounded to the engine dtype), in fp64.  centred: rows of different scales
    around zero; offset: unit spread around 10^4, where sums about zero lose eight digits of the variance."""
    rng = np.random.default_rng([seed, p, J, N, FAMILIES.index(family)])
    x = rng.standard_normal((N, p, J))
    if family == "centred":
        x = x * (10.0 ** rng.uniform(-2, 2, p))[None, :, None] + 0.3 * rng.standard_normal((1, p, J))
    else:
        x = 1e4 + x
    return x.astype(dtype).astype(np.float64)


def c_half(N):
    return N // 2 + 4


def slab_plan(p, J):
    """(chains per slab, slabs) of chain_pool_kernel: cs_slab_cols / cs_slabs of kernels_chainsum.hip."""
    t = -(-p // 64)
    pairs = t * (t + 1) // 2
    want = min(max(-(-WGS // pairs), -(-J // SLAB)), -(-J // TC))
    per = -(-J // want)
    cols = -(-per // TC) * TC
    return cols, -(-J // cols)


def plan_of(p, J):
    """The launch plan of the stage at an engine of p rows and J chains, from the kernel file's constants as ``slab_plan`` is:
    ``pairs`` (super tiles of the lower triangle: cs_pairs), ``cols`` and ``slabs`` (``slab_plan``), ``ntile`` (staged tiles a
    draw of the widest slab), ``last`` (chains of the last slab), ``slices`` (of the row sums behind c: cs_slices) and
    ``blocks`` (workgroups a row of chain_half_reduce_kernel: cs_blocks)."""
    t = -(-p // 64)
    cols, slabs = slab_plan(p, J)
    return dict(pairs=t * (t + 1) // 2, cols=cols, slabs=slabs, ntile=-(-min(J, cols) // TC), last=J - (slabs - 1) * cols,
                slices=max(1, min(SLICES, -(-J // 1024))), blocks=-(-J // CH))


def c_pool(N, J, p):
    cols, slabs = slab_plan(p, J)
    return min(N * min(J, cols) + slabs + N + 4, N * J + 8)


def c_shift(J):
    slices = max(1, min(64, -(-J // 1024)))
    per = -(-J // slices)
    return -(-per // 256) + 6 + 4 + slices + 4


def c_reduce(J):
    return 8 + 6 + 4 + -(-J // CH) + 4


def ref_raw(trace, c=None, mutant=None):
    """The raw sums of cesx_chain_summary_read of the draws ``trace`` (N, p, J), in numpy's extended precision and rounded to
    fp64 at the end, with B of every output (the same expression in absolute values) under the key ``B_<name>``.
    ``c``: the pooled shift to use (the device's own, so that both subtract the same number); None: the row mean of draw 0.
    ``mutant``: one of MUTANTS -- the reference made wrong on purpose, for the host test that the bounds see it."""
    L = np.longdouble
    x = np.asarray(trace, dtype=np.float64).astype(L)
    N, p, J = x.shape
    n = N // 2
    pooled = x
    if mutant == "draw_dropped":
        x = x[:-1]
        pooled = x
    c = np.asarray((x[0].sum(axis=1) / J) if c is None else c, dtype=np.float64).astype(L)     # an fp64 number, as the device's is
    shift = x[0]
    lo, hi = x[:n], x[N - n:]
    if mutant == "half_boundary_off_by_one":
        lo, hi = x[:n + 1], x[N - n + 1:]
    if mutant == "chain_left_out":                          # (J > 1)
        pooled = x[:, :, :-1]
    cols, _ = slab_plan(p, J)
    if mutant == "tile_dropped":                            # (cols > TC) the second staged tile of every slab never summed
        pooled = x[:, :, (np.arange(J) % cols) // TC != 1]
    if mutant == "chain_twice":                             # (slabs > 1) slab 0's ragged tile not zeroed past its j1
        pooled = np.concatenate([x, x[:, :, cols:cols + 1]], axis=2)
    S1 = np.stack([(h - shift).sum(axis=0) for h in (lo, hi)])
    S2 = np.stack([((h - shift) ** 2).sum(axis=0) for h in (lo, hi)])
    A1 = np.stack([np.abs(h - shift).sum(axis=0) for h in (lo, hi)])
    if mutant == "sums_about_zero":                         # no per-chain shift: S2 - S1^2 / n cancels |x|^2, in fp64 as a kernel would
        f1 = np.stack([h.astype(np.float64).sum(axis=0) for h in (lo, hi)])
        f2 = np.stack([(h.astype(np.float64) ** 2).sum(axis=0) for h in (lo, hi)])
        m = (f1 / n).astype(L)
        v = ((f2 - f1 * f1 / n) / (n - 1)).astype(L)
    else:
        m = (0 if mutant == "shift_not_added_back" else shift) + S1 / n
        v = (S2 - S1 * S1 / n) / (n - 1)
    Bm = np.abs(shift) + A1 / n
    Bv = (S2 + A1 * A1 / n) / (n - 1)
    d = pooled - c[None, :, None]
    s1 = d.sum(axis=(0, 2))
    cc = np.einsum("npj,nqj->pq", d, d)
    if mutant == "off_tile_uncentred":                      # (p > 64) the B panel of an off-diagonal super tile staged with c = 0
        cc[64:, :64] = np.einsum("npj,nqj->pq", d[:, 64:], pooled[:, :64])
    B_s1 = np.abs(d).sum(axis=(0, 2))
    B_cc = np.einsum("npj,nqj->pq", np.abs(d), np.abs(d))
    mm, vv = (m[:, :, :-1], v[:, :, :-1]) if mutant == "chain_left_out" else (m, v)
    H = mm.shape[0] * mm.shape[2]
    dm = mm - c[None, :, None]
    a0, a1 = dm.sum(axis=(0, 2)), (dm * dm).sum(axis=(0, 2))
    W = vv.sum(axis=(0, 2)) / H
    Bt = (a1 - a0 * a0 / H) / (H - 1)
    f = lambda a: np.asarray(a, dtype=np.float64)         # noqa: E731
    return dict(N=N, J=J, c=f(c), s1=f(s1), cc=np.tril(f(cc)), within=f(W), between=f(Bt), half_mean=f(m), half_var=f(v),
                B_c=f(np.abs(x[0]).sum(axis=1) / J), B_s1=f(B_s1), B_cc=np.tril(f(B_cc)), B_half_mean=f(Bm), B_half_var=f(Bv),
                a0_abs=f(np.abs(dm).sum(axis=(0, 2))), a1=f(a1), dm_abs=f(np.abs(dm)), v_abs=f(np.abs(vv)))


MUTANTS = ("draw_dropped", "half_boundary_off_by_one", "shift_not_added_back", "chain_left_out", "sums_about_zero",
           "tile_dropped", "chain_twice", "off_tile_uncentred")


def mutant_applies(name, p, J):
    """Whether the mutant ``name`` changes anything at an engine of p rows and J chains: the last three model a regime of the
    launch plan and are the reference itself where the plan does not reach it."""
    plan = plan_of(p, J)
    return {"chain_left_out": J > 1, "tile_dropped": plan["ntile"] > 1, "chain_twice": plan["slabs"] > 1,
            "off_tile_uncentred": plan["pairs"] > 1}.get(name, True)


def wb_bounds(ref):
    """(bound on W, bound on B_m) of a reference of ``ref_raw``: the terms' own errors through the sums, plus the reduce's."""
    N, J = ref["N"], ref["J"]
    H = 2 * J
    ch, c3 = c_half(N) * EPS, c_reduce(J) * EPS
    dm, dv = ch * ref["B_half_mean"], ch * ref["B_half_var"]
    dW = dv.sum(axis=(0, 2)) / H + c3 * ref["v_abs"].sum(axis=(0, 2)) / H
    da0 = dm.sum(axis=(0, 2)) + c3 * ref["a0_abs"]
    da1 = (2 * ref["dm_abs"] * dm).sum(axis=(0, 2)) + c3 * ref["a1"]
    dB = (da1 + 2 * ref["a0_abs"] * da0 / H) / (H - 1) + 4 * EPS * (ref["a1"] + ref["a0_abs"] ** 2 / H) / (H - 1)
    return dW, dB


def raw_bounds(ref):
    """{output: elementwise bound} for every output of cesx_chain_summary_read against ``ref_raw`` with the device's c."""
    N, J = ref["N"], ref["J"]
    cp, ch = c_pool(N, J, ref["c"].shape[0]) * EPS, c_half(N) * EPS
    dW, dB = wb_bounds(ref)
    return dict(s1=cp * ref["B_s1"], cc=cp * ref["B_cc"], half_mean=ch * ref["B_half_mean"], half_var=ch * ref["B_half_var"],
                within=dW, between=dB)


def finalise_ref(raw):
    """The summary dict from raw sums, written out from the issue's formulas (independent of ces_amd.sample.finalise_summary)."""
    N, J = raw["N"], raw["J"]
    T, n = N * J, N // 2
    cc = raw["cc"] + np.tril(raw["cc"], -1).T
    d = raw["s1"] / T
    W, B = raw["within"], raw["between"]
    vp = (n - 1) / n * W + B
    with np.errstate(divide="ignore", invalid="ignore"):
        return dict(n=N, chains=J, mean=raw["c"] + d, cov=(cc - T * np.outer(d, d)) / (T - 1), within=W, between=B,
                    rhat=np.sqrt(vp / W), ess=np.minimum(2.0 * J * n, 2.0 * J * vp / B))


def literal_summary(trace):
    """The summary of the draws ``trace`` (N, p, J) with numpy's own mean, cov and var: the issue's definitions, literally."""
    x = np.asarray(trace, dtype=np.float64)
    N, p, J = x.shape
    n = N // 2
    flat = x.transpose(1, 0, 2).reshape(p, N * J)
    halves = np.concatenate([x[:n], x[N - n:]], axis=2)    # (n, p, 2 J): every column a half-chain
    m, s2 = halves.mean(axis=0), halves.var(axis=0, ddof=1)
    W, B = s2.mean(axis=1), m.var(axis=1, ddof=1)
    vp = (n - 1) / n * W + B
    return dict(n=N, chains=J, mean=flat.mean(axis=1), cov=np.cov(flat, ddof=1).reshape(p, p), within=W, between=B,
                rhat=np.sqrt(vp / W), ess=np.minimum(2.0 * J * n, 2.0 * J * vp / B))


def summary_bounds(ref):
    """{key: bound} of the finalised dict against ``finalise_ref(ref)``: the raw bounds to first order, doubled."""
    N, J = ref["N"], ref["J"]
    T, n = N * J, N // 2
    rb = raw_bounds(ref)
    fin = finalise_ref(ref)
    d = np.abs(ref["s1"]) / T
    sym = lambda a: a + np.tril(a, -1).T                    # noqa: E731
    dcov = (sym(rb["cc"]) + np.outer(d, rb["s1"]) + np.outer(rb["s1"], d)) / (T - 1) \
        + 8 * EPS * (sym(ref["B_cc"]) + T * np.outer(d, d)) / (T - 1)
    W, B = ref["within"], ref["between"]
    vp = (n - 1) / n * W + B
    dvp = (n - 1) / n * rb["within"] + rb["between"]
    with np.errstate(divide="ignore", invalid="ignore"):
        drhat = fin["rhat"] * 0.5 * (dvp / vp + rb["within"] / W) + 8 * EPS * fin["rhat"]
        dess = 2.0 * J * (dvp / B + vp * rb["between"] / B ** 2) + 8 * EPS * 2.0 * J * vp / B
    out = dict(mean=rb["s1"] / T + 8 * EPS * (np.abs(ref["c"]) + d), cov=dcov, within=rb["within"], between=rb["between"],
               rhat=drhat, ess=dess)
    return {k: 2 * v for k, v in out.items()}


def draws_of(samples, n_mcmc, stride, burn):
    """The draws ``summary=True`` takes, from the twin call's ``samples`` (p, 1 + kept [+ 1], M) of a fresh run (or the new
    part of a resumed one, with the state it started from in front): (N, p, M)."""
    s = np.asarray(samples, dtype=np.float64)
    kept = s[:, 1:1 + n_mcmc // stride, :]                   # (the off-stride last state is not a draw)
    first = min(burn, n_mcmc) // stride                      # kept state t follows step stride (t + 1): > burn from here
    return np.ascontiguousarray(kept[:, first:, :].transpose(1, 0, 2))
