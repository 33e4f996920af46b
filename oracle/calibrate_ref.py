"""Staged fp64 references of the Calibrate stage's device steps: K1 (moments), K2 (dense algebra), K3 (update).

TEST INFRASTRUCTURE (see oracle/__init__.py).  Plain numpy restatements of what one kernel stage computes FROM THE VALUES
IT READS: the inputs already rounded to the engine dtype and, stage by stage, the device's own output of the stage
before (the moment buffer for K2; cesx_debug_dense and hk for K3; the drift of aldi_constant's first pass for its
second).  What is left between a kernel and its reference is the rounding of that kernel alone, so the comparison can be
ELEMENTWISE against a bound that arithmetic gives:

    |dev - ref| <= c * eps * B        for every entry,

eps the unit roundoff of the engine dtype (2^-24, 2^-53), B the reference's own expression with every matrix, vector and
scalar replaced by its absolute value and every minus by a plus (the sum of the magnitudes the kernel adds up), and c the
worst-case forward-error constant of the sums the kernel forms (Higham, Accuracy and Stability, section 3.1: a sum of m
products accumulated in any order has error <= gamma_m sum |a||b|, gamma_m ~ m eps, plus one eps for every operand that was
rounded before it entered).  c is DERIVED here, never fitted to what a device returns:

K3  c_update(p, n) = ktot + 8,  ktot = 2 pad16(p) + pad16(n) the padded depth of the [xi | U | G] product (include/cesx.h;
    cesx_internal.h, Engine::ktot).  The longest chain an output entry goes through is the whole k range in one fp32 / fp64
    MFMA accumulator: ktot additions.  In the chained form (kernels_update4.hip) the intermediate V = sqrt(2/hk) xi -
    L^T Sigma^{-1} U is a chain of pad16(p) + 1, L V another pad16(p), K G pad16(n): the same total.  The 8: one rounding
    of each coefficient to the engine dtype (the image is assembled in fp64 and stored rounded), one of sqrt(2 hk)/hk or
    1/hk + alpha, the rescale of the accumulators behind the xi segment, the rounding of the bias, its addition, the
    multiplication by hk, and (aldi_constant) the two epilogue products hk * drift and 1 * U with their additions.
    Launches with fewer segments (drift: [U | G]; finish: [xi]) have shorter chains; they are held to the same c.
    A dense Gamma adds the whitening launch G~ = L_Gamma^{-1} G in front (one more chain of pad16(n), its result rounded to
    the engine dtype and not readable through the ABI): c_update + pad16(n) + 2, with |K~| (|L_Gamma^{-1}| |G|) in B.
    The EKS form reads P = (I + hk M)^{-1} and P K, K2 products the ABI does not hand out either; the reference forms them
    itself and the bound carries BAND * B for them (the bar K2 is held to), in both dtypes.
K1  c_gram(chain) = chain + 4.  A Gram entry is sum_j fl(a_ij - s_i) fl(b_kj - s_k): two roundings of the shifted operands
    (and second-order terms: the 4), then the products accumulated in the engine dtype over the particles ONE SLAB holds
    before the fp64 reduce: ``chain``.  ``gram_chain`` takes it from the work partition (cesx_debug_gram_plan with the
    budgets cesx_create uses, from the device's CU count): a type's slices never exceed the J tiles, so the smallest type
    has at least workgroups - (types - 1) tiles slices and a slab at most ceil(tiles / that) tiles of 32 (fp32) / 16
    (fp64) particles.  One launch the host-only entry cannot reproduce: cesx_create re-plans the second fp32 launch with
    three types when the plan has two; for it the chain is all of J (the longest any partition can form).  The row sums
    sum_j fl(a_ij - s_i) are fp64 sums of once-rounded terms and are held to the same constant.
metrics  c_metric(n) = 2 (pad16(n) + 7) + 2.  q_j = sum_i w_i (g_ij - c_i)^2 in the engine dtype (chain pad16(n); c and w
    rounded to the engine dtype: 2 + 1; the difference, twice through the square: 2; the square and the product: 2), then
    q_j^2 and the sum over j in fp64: |d(q^2)| <= 2 q |dq| + dq^2.  Scale: mean_j (sum_i w_i (|g_ij| + |c_i|)^2)^2.
    A dense Gamma: the rows are those of G~ = L_Gamma^{-1} G from the whitening launch (a chain of pad16(n) and one rounding
    more per row, twice through the square: 2 (pad16(n) + 1) added inside the bracket), w = 1, c = L^{-1} y / L^{-1} gbar, and |g~| replaced by |L^{-1}| |G|.

The worst-case c is loose (hundreds); what keeps it from hiding a structural error is tests/test_calibrate_refs_host.py:
on every shape the GPU module runs, numpy IN THE ENGINE DTYPE stays below c eps B, and every mutant of ``mutants`` (one
term dropped, one entry off, one row / column / k-tile of one coefficient block zeroed, the last particles not updated)
exceeds 4 c eps B in at least one of the two problem families of ``family``.
"""
import numpy as np

BAND = 1e-9                      # the bar the project holds fp64 dense algebra to, relative to each array's maximum
EPS = {"float32": 2.0 ** -24, "float64": 2.0 ** -53}
FAMILIES = ("data", "prior")


def pad16(x):
    return (int(x) + 15) // 16 * 16


def ktot(p, n):
    return 2 * pad16(p) + pad16(n)


def c_update(p, n, dense_gamma=False):
    return ktot(p, n) + 8 + (pad16(n) + 2 if dense_gamma else 0)


def c_gram(chain):
    return int(chain) + 4


def gram_plans(p, n, J, dtype, cus, plan):
    """[(info, replanned)] of the two Gram launches of a single-device handle: ``plan(part, budget)`` is
    cesx_debug_gram_plan's info for this shape, the budgets are cesx_create's (all CUs; the second launch leaves 1 CU in 32
    free, 1 in 8 when chol(C) is the blocked one); replanned: the launch cesx_create plans again with three types."""
    slim = (p + 31) // 32 * 32 <= 256
    out = []
    for part, budget in ((0, cus), (1, cus - (cus // 32 if slim else cus // 8))):
        info = list(plan(part, budget))
        out.append((info, part == 1 and np.dtype(dtype) == np.float32 and info[0] == 2))
    return out


def gram_chain(p, n, J, dtype, cus, plan):
    """The most particles one slab accumulates in the engine dtype (module docstring, K1)."""
    kt = 32 if np.dtype(dtype) == np.float32 else 16
    ntiles = (J + kt - 1) // kt
    tiles = 1
    for info, replanned in gram_plans(p, n, J, dtype, cus, plan):
        types, wgs = info[0], info[1]
        if types == 0:
            continue
        tiles = max(tiles, ntiles if replanned else -(-ntiles // max(1, wgs - (types - 1) * ntiles)))
    return min(J, tiles * kt)


def c_metric(n, dense_gamma=False):
    return 2 * (pad16(n) + 7 + (2 * (pad16(n) + 1) if dense_gamma else 0)) + 2


def eps_of(dtype):
    return EPS[np.dtype(dtype).name]


def is_diagonal(A):
    A = np.asarray(A)
    return not np.count_nonzero(A - np.diag(np.diagonal(A)))


# ---- the two problem families -----------------------------------------------------------------------------------------

def _spd_with_diagonal(rng, d):
    """D^(1/2) (I + E / (2 ||E||_2)) D^(1/2), E the off-diagonal part of a Wishart draw: the diagonal is d, the correlation
    factor has its spectrum in [1/2, 3/2] (cond <= 3, so cond <= 3 max d / min d, far below the 1e2 asked for)."""
    m = len(d)
    B = rng.standard_normal((m, m))
    E = B @ B.T / m
    E = E - np.diag(np.diagonal(E))
    nrm = np.linalg.norm(E, 2)
    R = np.eye(m) + (0.5 / nrm) * E if nrm > 0 else np.eye(m)
    s = np.sqrt(d)
    return s[:, None] * R * s[None, :]


def family(name, p, n, J, dtype, seed=None, dense_gamma=False, dense_sigma=False, last=None):
    """One generated problem.  A = N(0,1)/sqrt(p), u* = N(0,1), y = A u* + 0.1 N(0,1), U0 = u* + 0.5 N(0,1),
    G = A U0 + 0.05 sin(A U0), xi = N(0,1); U0, G, xi rounded to the engine dtype (y, Gamma, mu, Sigma, u* cross the ABI
    as fp64).  'data': Gamma = 0.01 I, Sigma = 100 I, mu = 0 (data and noise carry the step).  'prior': Gamma = 10 diag(1 +
    r / 2), Sigma = diag(1 + r / 2), mu = 2 + 0.3 N(0,1), r uniform (the prior and alpha terms carry it).  dense_*: the same
    diagonals with an SPD off-diagonal part.  Seeded from the case's parameters (p + n + J unless a seed is given); both
    families of a seed share A, u*, y, U0, G, xi.
    last: factor on the LAST parameter's deviations from u*; None: 1, and 4 where J < p + 16.  With so few particles the
    trailing pivots of chol(C) are an order of magnitude below the others (the last Schur complement is var (J - p) / (J - 1)),
    and the one entry in the last row of L^T Sigma^{-1} then moves U_next by only 2.6 .. 4.0 times the bound at (225, 255,
    228), (249, 16, 252), (225, 1, 232) (measured on the host, tests/test_calibrate_refs_host.py; scaling the whole ensemble
    does not help, the bound scales with it).  A shape that cannot show a mutant gets other inputs, not an exemption."""
    if name not in FAMILIES:
        raise ValueError("unknown problem family %r" % (name,))
    dt = np.dtype(dtype)
    rng = np.random.default_rng(p + n + J if seed is None else seed)
    A = rng.standard_normal((n, p)) / np.sqrt(p)
    ustar = rng.standard_normal((p, 1))
    y = (A @ ustar).ravel() + 0.1 * rng.standard_normal(n)
    dev = 0.5 * rng.standard_normal((p, J))
    dev[-1] *= (4.0 if J < p + 16 else 1.0) if last is None else last
    U0 = ustar + dev
    G = A @ U0 + 0.05 * np.sin(A @ U0)
    xi = rng.standard_normal((p, J))
    rn, rp = rng.random(n), rng.random(p)
    mu = 2.0 + 0.3 * rng.standard_normal((p, 1))
    if name == "data":
        gd, sd, mu = np.full(n, 0.01), np.full(p, 100.0), np.zeros((p, 1))
    else:
        gd, sd = 10.0 * (1.0 + 0.5 * rn), 1.0 + 0.5 * rp
    Gamma = _spd_with_diagonal(rng, gd) if dense_gamma and n > 1 else np.diag(gd)
    sigma = _spd_with_diagonal(rng, sd) if dense_sigma and p > 1 else np.diag(sd)
    rd = lambda a: np.ascontiguousarray(a.astype(dt).astype(np.float64))       # noqa: E731
    return dict(A=A, ustar=ustar, y=y, Gamma=Gamma, sigma=sigma, mu=mu, U0=rd(U0), G=rd(G), xi=rd(xi))


# ---- K1 -------------------------------------------------------------------------------------------------------------------

def round_shift(sums, dtype):
    """set_shift_kernel: shift = (T)(sums[1 + row] / sums[0]), as fp64 values."""
    sums = np.asarray(sums, dtype=np.float64)
    return (sums[1:] / sums[0]).astype(np.dtype(dtype)).astype(np.float64)


def moments_layout(p, n):
    """Offsets of the packed buffer of include/cesx.h: N, sum a, S_aa | sum b, S_ab, S_bb, (two lagged metric sums)."""
    o = {"N": 0, "sa": 1, "Saa": 1 + p}
    o["sb"] = o["uu_len"] = 1 + p + p * p
    o["Sab"] = o["sb"] + n
    o["Sbb"] = o["Sab"] + p * n
    o["tail"] = o["Sbb"] + n * n
    o["len"] = o["tail"] + 2
    return o


def unpack(mom, p, n):
    mom = np.asarray(mom, dtype=np.float64)
    o = moments_layout(p, n)
    return dict(N=float(mom[0]), sa=mom[o["sa"]:o["Saa"]], Saa=mom[o["Saa"]:o["sb"]].reshape(p, p),
                sb=mom[o["sb"]:o["Sab"]], Sab=mom[o["Sab"]:o["Sbb"]].reshape(p, n),
                Sbb=mom[o["Sbb"]:o["tail"]].reshape(n, n))


def moments_ref(U, G, s_u, s_g):
    """(buffer, scale): the packed moment buffer without its two lagged entries from fp64 sums of the shifted data, and
    the same sums of absolute values (sum_j |a_ij - s_i| |b_kj - s_k|; 0 for N, which is exact)."""
    U, G = np.asarray(U, dtype=np.float64), np.asarray(G, dtype=np.float64)
    a = U - np.asarray(s_u, dtype=np.float64).reshape(-1, 1)
    b = G - np.asarray(s_g, dtype=np.float64).reshape(-1, 1)
    return _pack(a, b, float(U.shape[1])), _pack(np.abs(a), np.abs(b), 0.0)


def _pack(a, b, N):
    return np.concatenate([[N], a.sum(axis=1), (a @ a.T).ravel(), b.sum(axis=1), (a @ b.T).ravel(), (b @ b.T).ravel()])


def moments_in_dtype(U, G, s_u, s_g, dtype, chain):
    """The buffer the way the kernels form it, by numpy: operands shifted in the engine dtype, products summed in it over
    slabs of ``chain`` particles, the slabs and the row sums in fp64 (condition (a) of the host test)."""
    dt = np.dtype(dtype)
    a = np.asarray(U, dtype=np.float64).astype(dt) - np.asarray(s_u, dtype=np.float64).astype(dt).reshape(-1, 1)
    b = np.asarray(G, dtype=np.float64).astype(dt) - np.asarray(s_g, dtype=np.float64).astype(dt).reshape(-1, 1)
    J = a.shape[1]
    out = 0.0
    for j0 in range(0, J, chain):
        sa, sb = a[:, j0:j0 + chain], b[:, j0:j0 + chain]
        out = out + np.concatenate([[0.0], sa.sum(axis=1, dtype=np.float64), (sa @ sa.T).ravel().astype(np.float64),
                                    sb.sum(axis=1, dtype=np.float64), (sa @ sb.T).ravel().astype(np.float64),
                                    (sb @ sb.T).ravel().astype(np.float64)])
    out[0] = float(J)
    return out


def moments_mutants(U, G, s_u, s_g, kt):
    """{name: buffer} of the K1 reference with one thing wrong -- for the host test alone: the last particle or the last J
    tile of kt particles left out of every sum, and one particle too many (a zero column past J that is shifted and summed)."""
    U, G = np.asarray(U, dtype=np.float64), np.asarray(G, dtype=np.float64)
    J = U.shape[1]
    last = J - ((J - 1) // kt) * kt
    out = {"last_particle_dropped": moments_ref(U[:, :-1], G[:, :-1], s_u, s_g)[0],
           "last_tile_dropped": moments_ref(U[:, :J - last], G[:, :J - last], s_u, s_g)[0],
           "padding_column_summed": moments_ref(np.hstack([U, np.zeros((U.shape[0], 1))]), np.hstack([G, np.zeros((G.shape[0], 1))]), s_u, s_g)[0]}
    for m in out.values():
        m[0] = float(J)
    return out


# ---- K2 -------------------------------------------------------------------------------------------------------------------

def whitening(Gamma):
    """(L, L^{-1}) of a dense Gamma = L L^T, or (None, None) for a diagonal one (the engine whitens only then)."""
    Gamma = np.asarray(Gamma, dtype=np.float64)
    if is_diagonal(Gamma):
        return None, None
    Lg = np.linalg.cholesky(Gamma)
    return Lg, np.linalg.solve(Lg, np.eye(len(Lg)))


def dense_ref(mom, shift, prob, update, time_step=None, delta_t=None, spinup=4.0, first_step=True, t_len=0, t_last=0.0, T=30):
    """K2 from the (device's) moment buffer and the centring shift it was taken with.  With a dense Gamma the buffer and
    the G part of the shift are those of the whitened data G~ = L^{-1} G (include/cesx.h); gbar and K are returned in the
    caller's coordinates as cesx_debug_dense reports them.  hk, t are None for aldi_constant (they need max|drift|)."""
    p, n = len(np.asarray(prob["mu"]).ravel()), len(np.asarray(prob["y"]).ravel())
    m = unpack(mom, p, n)
    N = m["N"]
    shift = np.asarray(shift, dtype=np.float64)
    Lg, Li = whitening(prob["Gamma"])
    y = np.asarray(prob["y"], dtype=np.float64).ravel()
    if Lg is None:
        yw, Gw = y, np.asarray(prob["Gamma"], dtype=np.float64)
    else:
        yw, Gw = Li @ y, np.eye(n)
    ubar = shift[:p] + m["sa"] / N
    gbar_w = shift[p:] + m["sb"] / N
    S_uu = m["Saa"] - np.outer(m["sa"], m["sa"]) / N
    C = S_uu / (N if update == "eks" else N - 1.0) + 1e-8 * np.eye(p)
    Cug = (m["Sab"] - np.outer(m["sa"], m["sb"]) / N) / N
    See = m["Sbb"] - np.outer(m["sb"], m["sb"]) / N
    mv = gbar_w - yw
    Srr = See + N * np.outer(mv, mv)
    X = np.linalg.solve(Gw, Srr)
    X = np.linalg.solve(Gw, X.T).T
    frob = np.sqrt(max(float((X * See).sum()), 0.0)) / N
    sigma = np.asarray(prob["sigma"], dtype=np.float64)
    M = np.linalg.solve(sigma.T, C.T).T
    L = np.linalg.cholesky(C)
    ustar = np.asarray(prob["ustar"], dtype=np.float64).ravel()
    out = dict(ubar=ubar, C=C, L=L, M=M, alpha=(p + 1.0) / N, self_bias=float(np.trace(S_uu)) / N, radspec=None, hk=None, t=None)
    out["bias"] = out["self_bias"] + float(((ubar - ustar) ** 2).sum())
    if update == "aldi_constant":
        Kw = np.linalg.solve(Gw.T, Cug.T).T
    else:
        if time_step is None:
            hk = 1.0 / (frob + 1e-8)
        elif time_step == "spectral":
            out["radspec"] = max(float(np.linalg.eigvals(np.linalg.solve(Gw, See) / N).real.max()), 0.0)
            hk = 1.0 / out["radspec"]
        elif time_step == "constant":
            hk = delta_t if delta_t is not None else 1.0 / (T / 2)
        elif time_step == "mix":
            hk = 1.0 / (frob + 1e-8) if (t_len == 0 or t_last < spinup) else (delta_t if delta_t is not None else 1.0 / (T / 2))
        else:
            raise ValueError("no reference for time_step %r" % (time_step,))
        out["hk"], out["t"] = hk, (hk if first_step else hk + t_last)
        recompute = time_step == "constant" or (update == "aldi" and time_step == "mix" and out["t"] > 1)
        Kw = np.linalg.solve((hk * (See / N) + Gw if recompute else Gw).T, Cug.T).T
    out["K"] = Kw if Lg is None else Kw @ Li
    out["gbar"] = gbar_w if Lg is None else Lg @ gbar_w
    return out


def dense_from_inputs(U, G, prob, update, dtype, **ts):
    """K2 from a step's OWN inputs (no device buffer in it): the fp64 moments of U and G -- with a dense Gamma of the whitened
    rows L_Gamma^{-1} G -- about the dtype-rounded row means, through ``dense_ref``.  ubar, gbar, C, K, M and the scalars do not
    depend on the shift in exact arithmetic, so any engine shift (recomputed or predicted) is held to the same reference; what
    separates a device from it is the Gram rounding of the engine dtype (tests/reuse_cases.py: BAND for an fp64
    engine, the project's fp32 bar for an fp32 one).  ts: the keywords of ``dense_ref``."""
    U, G = np.asarray(U, dtype=np.float64), np.asarray(G, dtype=np.float64)
    p, J = U.shape
    Lg, Li = whitening(prob["Gamma"])
    Gw = G if Lg is None else Li @ G
    shift = round_shift(np.concatenate([[float(J)], U.sum(axis=1), Gw.sum(axis=1)]), dtype)
    mom, _ = moments_ref(U, Gw, shift[:p], shift[p:])
    return dense_ref(mom, shift, prob, update, **ts)


# ---- K3 -------------------------------------------------------------------------------------------------------------------

FORMS = ("assembled", "hkfree", "chained", "eks", "drift", "finish")
FORM_BLOCKS = {"assembled": ("L", "M", "K"), "hkfree": ("L", "M", "K"), "chained": ("L", "N", "K"), "eks": ("L", "P", "PK"),
               "drift": ("M", "K"), "finish": ("L",)}
FORM_OF_UPDATE_FORM = {0: "assembled", 1: "hkfree", 2: "chained"}      # cesx_debug_update_form of an ALDI step


def _parts(form, dd, hk, prob, J, switch=1.0, drop_prior=False, drop_mu=False, sinv_last=1.0, alpha_zero=False):
    """The coefficient blocks and vectors of one launch, fp64, from the device's dense state."""
    p = len(dd["ubar"])
    sigma = np.asarray(prob["sigma"], dtype=np.float64).reshape(p, p)
    Sinv = np.linalg.inv(sigma)
    C, L, K = (np.asarray(dd[k], dtype=np.float64) for k in ("C", "L", "K"))
    L = np.tril(L)
    M = np.asarray(dd["M"], dtype=np.float64)
    if sinv_last != 1.0:
        Sinv = Sinv.copy()
        Sinv[-1, -1] *= sinv_last
        M = C @ Sinv
    N = -(L.T @ Sinv)                     # the chained image's -L^T Sigma^{-1} (a diagonal Sigma: upper triangular)
    if drop_prior:
        M, N = np.zeros_like(M), np.zeros_like(N)
    mu = np.zeros(p) if drop_mu else np.asarray(prob["mu"], dtype=np.float64).ravel()
    y = np.asarray(prob["y"], dtype=np.float64).ravel()
    alpha = 0.0 if alpha_zero else (p + 1.0) / J
    if form == "drift":
        alpha = switch * alpha
    P = dict(L=L, M=M, N=N, K=K, alpha=alpha, noise=1.0, ubar=np.asarray(dd["ubar"], dtype=np.float64), mu=mu, y=y, hk=hk)
    if form == "eks":
        P["P"] = np.linalg.inv(np.eye(p) + hk * M)
        P["PK"] = P["P"] @ K
    Lg, Li = whitening(prob["Gamma"])
    P["Kw"], P["Li"] = (None, None) if Lg is None else (K @ Lg, Li)
    return P


def _eval(form, P, U, G, xi, drift=None, ab=False, dt=None):
    """One launch.  ab: the bound's scale B (absolute values, minus -> plus).  dt: evaluated in that dtype the way the kernels
    do (coefficients formed in fp64 and rounded, products and sums in dt), for condition (a) of the host test."""
    a = np.abs if ab else (lambda x: x)
    sg = 1.0 if ab else -1.0
    if dt is None:
        r = lambda x: np.asarray(x, dtype=np.float64)                                  # noqa: E731
    else:
        r = lambda x: np.asarray(x, dtype=np.float64).astype(dt)                       # noqa: E731
    hk, al, nz = P["hk"], P["alpha"], P["noise"]
    p = len(P["ubar"])
    I = np.eye(p)
    col = lambda v: r(v)[:, None]                                                      # noqa: E731
    U_, G_, X_ = (None if x is None else r(a(np.asarray(x, dtype=np.float64))) for x in (U, G, xi))

    def KG():             # K G, or with a dense Gamma K~ G~ with G~ = L^{-1} G from the whitening launch (rounded to dt there)
        if P["Kw"] is None or not (ab or dt is not None):
            return r(a(P["K"])) @ G_
        return r(a(P["Kw"])) @ r(r(a(P["Li"])) @ G_)

    def Kvec(v):          # K v for the bias (fp64 on the device)
        return a(P["K"]) @ a(v)

    if form in ("assembled", "hkfree", "chained", "drift"):
        bp = Kvec(P["y"]) + a(P["M"]) @ a(P["mu"]) + sg * al * a(P["ubar"])            # K y + M mu - alpha ubar
    if form == "assembled":
        s2 = np.sqrt(2.0 * hk)
        Wu = (1.0 + hk * al) * I + sg * hk * a(P["M"])
        return r(Wu) @ U_ + sg * (r(hk * a(P["K"])) @ G_ if P["Kw"] is None else hk * KG()) + r(nz * s2 * a(P["L"])) @ X_ + col(hk * bp)
    if form == "hkfree":
        Du = (al + 1.0 / hk) * I + sg * a(P["M"])
        acc = (r(a(P["L"])) @ X_) * r(nz * np.sqrt(2.0 * hk) / hk)
        acc = acc + r(Du) @ U_ + sg * KG()
        return r(hk) * (acc + col(bp))
    if form == "chained":
        V = r(nz * np.sqrt(2.0 * hk) / hk) * X_ + r(a(P["N"])) @ U_
        O = r(a(P["L"])) @ V + r(1.0 / hk + al) * U_ + sg * KG() + col(bp)
        return r(hk) * O
    if form == "eks":
        s2 = np.sqrt(2.0 * hk)
        b = a(P["P"]) @ (hk * (Kvec(P["y"]) + a(P["M"]) @ a(P["mu"])))
        PKG = r(hk * a(P["PK"])) @ G_ if P["Kw"] is None or not (ab or dt is not None) else \
            r(hk * a(P["P"] @ P["Kw"])) @ r(r(a(P["Li"])) @ G_)
        return r(a(P["P"])) @ U_ + sg * PKG + r(nz * s2 * a(P["L"])) @ X_ + col(b)
    if form == "drift":
        Wd = al * I + sg * a(P["M"])
        return r(Wd) @ U_ + sg * KG() + col(bp)
    if form == "finish":
        D_ = r(a(np.asarray(drift, dtype=np.float64)))
        return r(nz * np.sqrt(2.0 * hk) * a(P["L"])) @ X_ + U_ + r(hk) * D_
    raise ValueError("unknown form %r" % (form,))


def update_ref(form, dd, hk, U, G, xi, prob, J=None, switch=1.0, drift=None):
    """(ref, B) of one update launch in the form the kernel executes (FORMS):
    assembled  W [U; G; xi] + b,  W = [(1 + hk a) I - hk M | -hk K | sqrt(2hk) L],  b = hk (K y + M mu - a ubar)
    hkfree     hk (sqrt(2/hk) L xi + (a I - M + I/hk) U - K G + b'),                b' = K y + M mu - a ubar
    chained    hk ((1/hk + a) U + L (sqrt(2/hk) xi - L^T Sigma^{-1} U) - K G + b')
    eks        [P | -hk P K | sqrt(2hk) L] [U; G; xi] + P hk (K y + M mu),          P = (I + hk M)^{-1}
    drift      [switch a I - M | -K] [U; G] + K y + M mu - switch a ubar            (aldi_constant, first pass)
    finish     sqrt(2hk) L xi + U + hk drift                                        (second pass, hk = 0.1 / max|drift|)
    dd: cesx_debug_dense of the step (ubar, C, L, K, M); J the global ensemble size (alpha = (p + 1) / J)."""
    J = np.asarray(U).shape[1] if J is None else J
    P = _parts(form, dd, hk, prob, J, switch=switch)
    return _eval(form, P, U, G, xi, drift), _eval(form, P, U, G, xi, drift, ab=True)


def update_in_dtype(form, dd, hk, U, G, xi, prob, dtype, J=None, switch=1.0, drift=None):
    """The unmutated form evaluated by numpy in ``dtype`` (condition (a): the engine dtype; numpy's extended precision gives
    an fp64 engine its reference).  Returned in that dtype when it is wider than fp64."""
    J = np.asarray(U).shape[1] if J is None else J
    P = _parts(form, dd, hk, prob, J, switch=switch)
    dt = np.dtype(dtype)
    return np.asarray(_eval(form, P, U, G, xi, drift, dt=dt), dtype=dt if dt.itemsize > 8 else np.float64)


def _zero(A, what):
    A = A.copy()
    if what == "last_row":
        A[-1, :] = 0.0
    elif what == "last_col":
        A[:, -1] = 0.0
    else:
        A[:, 16 * ((A.shape[1] - 1) // 16):] = 0.0
    return A


def mutants(form, dd, hk, U, G, xi, prob, J=None, switch=1.0, drift=None):
    """{name: U_next} of the reference with ONE thing wrong -- for the host test alone (never compared with a device)."""
    J = np.asarray(U).shape[1] if J is None else J
    U = np.asarray(U, dtype=np.float64)
    out = {}

    def run(name, P):
        out[name] = _eval(form, P, U, G, xi, drift)

    def parts(**kw):
        return _parts(form, dd, hk, prob, J, switch=switch, **kw)
    if form != "finish":
        run("prior_dropped", parts(drop_prior=True))
        run("mu_dropped", parts(drop_mu=True))
        run("sigma_inv_last_entry_1pct", parts(sinv_last=1.01))
    if form in ("assembled", "hkfree", "chained", "drift"):
        run("alpha_zero", parts(alpha_zero=True))
    if form not in ("drift",):
        P = parts()
        P["noise"] = 1.05
        run("noise_5pct", P)
    for blk in FORM_BLOCKS[form]:
        for what in ("last_row", "last_col", "last_ktile"):
            P = parts()
            P[blk] = _zero(P[blk], what)
            if blk == "K" and P["Kw"] is not None:
                P["Kw"] = _zero(P["Kw"], what)
            run("%s_%s" % (blk, what), P)
    good = _eval(form, parts(), U, G, xi, drift)
    base = np.asarray(drift, dtype=np.float64) if form == "drift" and drift is not None else U
    for k in (1, 4):
        m = good.copy()
        m[:, -k:] = 0.0 if form == "drift" else base[:, -k:]
        out["last_%d_particles_not_updated" % k] = m
    return out


# ---- the per-particle data metrics (summed inside K3) ---------------------------------------------------------------------

def data_metrics_ref(G, gbar, y, gw, J_global=None, G_abs=None):
    """{'bias_data': (value, scale), 'self_bias_data': (value, scale)}: mean_j (sum_i w_i (g_ij - c_i)^2)^2 with c = y /
    gbar, from fp64 sums of the rounded G (a diagonal Gamma: w = 1 / Gamma_ii); scale as in the module docstring.  G_abs:
    what stands for |G| in the scale (a dense Gamma: G is L^{-1} G in fp64 and G_abs is |L^{-1}| |G|)."""
    G = np.asarray(G, dtype=np.float64)
    J = G.shape[1] if J_global is None else J_global
    w = np.asarray(gw, dtype=np.float64).reshape(-1, 1)
    out = {}
    for key, c in (("bias_data", y), ("self_bias_data", gbar)):
        c = np.asarray(c, dtype=np.float64).reshape(-1, 1)
        q = (w * (G - c) ** 2).sum(axis=0)
        qa = (w * ((np.abs(G) if G_abs is None else G_abs) + np.abs(c)) ** 2).sum(axis=0)
        out[key] = (float((q * q).sum() / J), float((qa * qa).sum() / J))
    return out
