"""The dense per-chain likelihood on the device (CESX_GP_DENSE, gp_score_dense_kernel; gp_mh(chains=, pca_tools=)).

The score is held ELEMENTWISE, through cesx_mh_phi: gp_start('dense') on crafted mean and variance rows (not through the
GP), then the chains' phi against the literal reference of tests/gp_dense_cases.py within its bound_j (the bar and the
measurement behind its constant are in that module).  The accept loop runs through run_accept_steps of
tests/test_gpu_sample_edges.py with the band max(1e-9 max(1, |phi|), bound(U) + bound(P)) and the cap of 1 chain-step in
1000 left out; guards around every buffer the kernel may write.

Worst |phi - reference| / bound_j per part is printed (pytest -s) and recorded in NOTEBOOK.md."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gp_dense_cases as gc  # noqa: E402
from edge_helpers import guarded, guards_intact, put, same_bits  # noqa: E402
from test_emulate_host import gold_prior, gold_problem, load_gold  # noqa: E402
from test_gpu_sample_edges import SEED, eng_mod, note, run_accept_steps  # noqa: E402,F401

from oracle import stage_ref as sr  # noqa: E402

pytestmark = pytest.mark.gpu

BETA = 0.3
STEPS = 8


def trivial_image(p, k):
    """The smallest emulator cesx_gp_set takes: mode 'dense' needs one installed with n_gp = k and reads none of it."""
    return dict(n=k, Jt=1, p=p, A=np.tile(np.eye(p), (k, 1, 1)), c=np.zeros(p), Z=np.zeros((k, 1, p)),
                family=np.zeros(k, dtype=np.int32), par=np.tile([1.0, 0.1, 0.0], (k, 1)), mw=np.zeros((k, p)),
                alpha=np.zeros((k, 1)), Li=np.ones((k, 1, 1)))


def dense_engine(eng_mod, pr, M, dtype, kind, logdet, **kw):
    eng = eng_mod.Engine(pr["p"], pr["n"], M, dtype=dtype, **kw)
    eng.set_problem(pr["y"], pr["Gamma"], pr["mu"], pr["Sp"], pr["mu"])
    S = 0.3 * np.linalg.cholesky(pr["Sp"])
    eng.mh_set_proposal(kind, S, BETA)
    eng.gp_set(trivial_image(pr["p"], pr["k"]))
    eng.gp_dense_set(pr["B"], pr["g0"], logdet)
    return eng, S


def dev(eng, a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=eng.device)


def start_and_read(eng, U, Uh, m, v):
    """gp_start('dense') on the rows, the chains' phi back; the states untouched."""
    put(U, Uh)
    md, vd = dev(eng, m), dev(eng, v)
    eng.gp_start("dense", U, md, vd)
    phi = eng.mh_phi()
    assert np.all(same_bits(U.cpu().numpy(), Uh))
    assert np.array_equal(md.cpu().numpy(), m) and np.array_equal(vd.cpu().numpy(), v)
    return phi


# ---- the score, elementwise ----------------------------------------------------------------------------------------------

# (M, logdet, dense prior, update, dtype): every shape meets every chain count, both log det values, both priors, both
# updates and both engine dtypes
VARIANTS = [(1, True, True, None, "float32"), (5, False, False, "pCN", "float64"), (257, True, False, None, "float64"),
            (5, True, True, "pCN", "float32"), (1, False, False, None, "float64"), (257, False, True, "pCN", "float32")]


def test_the_variants_cover_what_they_must():
    assert {v[0] for v in VARIANTS} == set(gc.GPU_M)
    for col, vals in ((1, {True, False}), (2, {True, False}), (3, {None, "pCN"}), (4, {"float64", "float32"})):
        assert {v[col] for v in VARIANTS} == vals
    assert {(v[1], v[4]) for v in VARIANTS} == {(a, b) for a in (True, False) for b in ("float64", "float32")}


@pytest.mark.parametrize("n,k", gc.GPU_SHAPES)
def test_score_elementwise(eng_mod, n, k):
    for vi, (M, logdet, dense_prior, kind, dtype) in enumerate(VARIANTS):
        rng = np.random.default_rng([n, k, vi])
        pr = gc.problem(rng, n, k, 1e4 if n > 1 else 1, "pca", dense_prior=dense_prior)
        eng, _ = dense_engine(eng_mod, pr, M, dtype, kind, logdet)
        U_flat, U = guarded(eng, pr["p"])
        Uh = gc.states(rng, pr, M, np.dtype(dtype))
        m, v = gc.rows(rng, k, M)
        phi = start_and_read(eng, U, Uh, m, v)
        want, bound, cond, _ = gc.reference(pr, m, v, Uh.astype(np.float64), logdet)
        assert np.all(cond <= gc.COND_SCORE), cond.max()
        ratio = float(np.max(np.abs(phi - want) / bound))
        w = note("dense score", ratio=ratio)
        print("gp_start dense %s n=%d k=%d M=%d logdet=%d %s prior %s: cond_2 up to %.1e, worst |phi - ref| / bound %.3g "
              "(so far %.3g)" % (dtype, n, k, M, logdet, "dense" if dense_prior else "diagonal", kind or "RW", cond.max(),
                                 ratio, w["ratio"]))
        assert np.all(np.abs(phi - want) <= bound), (vi, ratio, np.flatnonzero(~(np.abs(phi - want) <= bound))[:8])
        assert guards_intact(U_flat, U)
        nsteps, rate, per = eng.mh_stats(per_chain=True)
        assert nsteps == 0 and rate == 0.0 and not per.any()


def test_compounded_dense_gamma_through_the_identity(eng_mod):
    """B = I, g0 = 0: Sigma = Gamma + diag(v), the dense compounded likelihood of ces/sample.py:50-51."""
    n, M = 50, 33
    rng = np.random.default_rng(50)
    pr = gc.problem(rng, n, n, 1e4, "cmp")
    pr["g0"] = np.zeros(n)
    eng, _ = dense_engine(eng_mod, pr, M, "float64", None, True)
    U_flat, U = guarded(eng, pr["p"])
    Uh = gc.states(rng, pr, M)
    m, v = gc.rows(rng, n, M)
    m = pr["y"][:, None] + 0.1 * m
    phi = start_and_read(eng, U, Uh, m, v)
    want, bound, _, _ = gc.reference(pr, m, v, Uh, True)
    lit = np.array([0.5 * (m[:, j] - pr["y"]) @ np.linalg.solve(pr["Gamma"] + np.diag(v[:, j]), m[:, j] - pr["y"])
                    + 0.5 * np.linalg.slogdet(pr["Gamma"] + np.diag(v[:, j]))[1] for j in range(M)]) + gc.prior_term(pr, Uh)[0]
    assert np.all(np.abs(want - lit) <= bound)
    assert np.all(np.abs(phi - want) <= bound), float(np.max(np.abs(phi - want) / bound))


# ---- the accept loop -----------------------------------------------------------------------------------------------------

def accept_case(eng_mod, n, k, M, dtype, kind, dense_prior, logdet, uniform=None, bad_chain=None, part="dense accept"):
    ndt = np.dtype(dtype)
    rng = np.random.default_rng([n, k, M, 1 if dtype == "float32" else 0, 1 if kind else 0, int(dense_prior), int(logdet)])
    pr = gc.problem(rng, n, k, 1e2 if n > 1 else 1, "pca", dense_prior=dense_prior, b_scale=(-2.0, 0.0))
    p = pr["p"]
    kw, step_ids = {}, list(range(STEPS))
    if uniform is not None:
        seed, j_offset, step_ids = uniform
        kw = dict(seed=seed, j_offset=j_offset, J_global=j_offset + M)
    eng, S = dense_engine(eng_mod, pr, M, dtype, kind, logdet, **kw)

    def ref_of(Xh, m, v):
        ph, b, cond, _ = gc.reference(pr, m, v, Xh.astype(np.float64), logdet)
        assert np.all(cond[np.isfinite(cond)] <= gc.COND_ACCEPT)
        return ph, b

    U_flat, U = guarded(eng, p)
    P_flat, P = guarded(eng, p)
    Uh = gc.states(rng, pr, M, ndt)
    m0, v0 = gc.rows(rng, k, M, v_lo=1e-6)
    phi_dev = start_and_read(eng, U, Uh, m0, v0)
    phi0, b0 = ref_of(Uh, m0, v0)
    assert np.all(np.abs(phi_dev - phi0) <= b0) and guards_intact(U_flat, U)
    ref = gc.DenseAcceptRef(phi0, b0)
    U0 = Uh.copy()
    keep = [None, None]

    def make_step(i, Uh):
        Ph = sr.propose(Uh.astype(np.float64), S, rng.standard_normal((p, M)), kind, BETA).astype(ndt)
        m, v = gc.rows(rng, k, M, v_lo=1e-6)
        logu = np.log(rng.random(M)) if uniform is None else sr.log_uniform(M, seed, step_ids[i], j_offset)
        if bad_chain is not None:                           # Sigma indefinite in this chain's proposal; any finite phi would pass
            v[i % k, bad_chain] = -10.0
            logu[bad_chain] = -1e6
            assert np.linalg.eigvalsh(gc.sigma_of(pr, v[:, bad_chain])).min() < 0.0
        phi_p, b_p = ref_of(Ph, m, v)
        return dict(P=Ph, m=m, v=v, phi_p=phi_p, logu=logu, half_width=ref.half_width(b_p))

    def launch(step, d):
        put(P, d["P"])
        keep[:] = [dev(eng, d["m"]), dev(eng, d["v"])]
        lu = None if uniform is not None else dev(eng, d["logu"])
        eng.gp_accept("dense", step, U, P, keep[0], keep[1], logu=lu)
        assert np.all(same_bits(P.cpu().numpy(), d["P"]))

    label = "gp_accept dense %s n=%d k=%d M=%d %s %s prior logdet=%d%s%s" % (
        dtype, n, k, M, kind or "RW", "dense" if dense_prior else "diagonal", logdet,
        " device uniform j_offset=%d" % uniform[1] if uniform else "", " indefinite proposals" if bad_chain is not None else "")
    Uh, taken = run_accept_steps(eng, U_flat, U, Uh, ref, step_ids, make_step, launch, label, part)
    assert guards_intact(P_flat, P)
    # the chains' phi after the loop: the reference's, within the bound of the state each chain holds
    phi_end = eng.mh_phi()
    assert np.all(np.abs(phi_end - ref.phi) <= ref.bound), float(np.max(np.abs(phi_end - ref.phi) / ref.bound))
    if M >= 33:
        assert 0 < taken < len(step_ids) * M, (label, taken)
    if bad_chain is not None:
        assert ref.count[bad_chain] == 0 and np.all(same_bits(Uh[:, bad_chain], U0[:, bad_chain]))
    return ref


ACCEPT_CASES = [(1, 1, 5, "float64", None, False, True), (2, 2, 257, "float32", "pCN", True, True),
                (63, 3, 257, "float64", "pCN", True, False), (64, 64, 130, "float32", None, False, True),
                (65, 1, 257, "float64", None, True, True), (127, 3, 33, "float32", "pCN", False, False),
                (128, 128, 33, "float64", None, False, True)]


@pytest.mark.parametrize("n,k,M,dtype,kind,dense_prior,logdet", ACCEPT_CASES)
def test_accept_loop(eng_mod, n, k, M, dtype, kind, dense_prior, logdet):
    accept_case(eng_mod, n, k, M, dtype, kind, dense_prior, logdet)


def test_accept_with_the_device_uniform(eng_mod):
    steps = [0, 1, 2, 3, 4, 5, 6, 2 ** 31 - 1]
    accept_case(eng_mod, 65, 3, 257, "float64", None, False, True, uniform=(SEED, 2 ** 32 + 7, steps), part="dense uniform")


# ---- an indefinite Sigma -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_an_indefinite_sigma_is_nan_and_rejects(eng_mod, dtype):
    n, k, M, bad = 65, 3, 70, 37
    rng = np.random.default_rng([65, 3, 1 if dtype == "float32" else 0])
    pr = gc.problem(rng, n, k, 1e2, "pca", b_scale=(-2.0, 0.0))
    eng, S = dense_engine(eng_mod, pr, M, dtype, None, True)
    U_flat, U = guarded(eng, pr["p"])
    P_flat, P = guarded(eng, pr["p"])
    Uh = gc.states(rng, pr, M, np.dtype(dtype))
    m, v = gc.rows(rng, k, M, v_lo=1e-6)
    v[1, bad] = -10.0
    assert np.linalg.eigvalsh(gc.sigma_of(pr, v[:, bad])).min() < 0.0
    phi = start_and_read(eng, U, Uh, m, v)
    want, bound, _, _ = gc.reference(pr, m, v, Uh.astype(np.float64), True)
    good = np.arange(M) != bad
    assert np.isnan(phi[bad]) and np.isnan(want[bad])
    assert np.all(np.abs(phi[good] - want[good]) <= bound[good])
    # the start state is stuck: a proposal any finite phi would take is refused
    Ph = sr.propose(Uh.astype(np.float64), S, rng.standard_normal((pr["p"], M))).astype(Uh.dtype)
    put(P, Ph)
    m2, v2 = gc.rows(rng, k, M, v_lo=1e-6)
    md, vd = dev(eng, m2), dev(eng, v2)
    eng.gp_accept("dense", 0, U, P, md, vd, logu=dev(eng, np.full(M, -1e6)))
    Un = U.cpu().numpy()
    assert np.all(same_bits(Un[:, bad], Uh[:, bad])) and np.all(same_bits(Un[:, good], Ph[:, good]))
    _, _, per = eng.mh_stats(per_chain=True)
    assert per[bad] == 0 and np.all(per[good] == 1)
    assert np.isnan(eng.mh_phi()[bad]) and guards_intact(U_flat, U) and guards_intact(P_flat, P)
    # ... and an indefinite PROPOSAL is rejected by a chain with a finite phi, through the loop's own checks
    accept_case(eng_mod, n, k, M, dtype, None, False, True, bad_chain=bad, part="dense indefinite")


# ---- determinism ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,k", [(65, 3), (128, 128)])
def test_bits_do_not_depend_on_the_call_the_column_or_the_neighbours(eng_mod, n, k):
    rng = np.random.default_rng([n, k, 9])
    pr = gc.problem(rng, n, k, 1e4, "pca", dense_prior=True)
    M = 257
    Uh = gc.states(rng, pr, M)
    m, v = gc.rows(rng, k, M)
    for col in (64, 256):                                    # the same chain data at columns 0, 64 and 256
        Uh[:, col], m[:, col], v[:, col] = Uh[:, 0], m[:, 0], v[:, 0]
    eng, _ = dense_engine(eng_mod, pr, M, "float64", None, True)
    _, U = guarded(eng, pr["p"])
    one = start_and_read(eng, U, Uh, m, v)
    two = start_and_read(eng, U, Uh, m, v)
    assert np.all(same_bits(one, two))
    assert same_bits(one[[0]], one[[64]])[0] and same_bits(one[[0]], one[[256]])[0]
    eng1, _ = dense_engine(eng_mod, pr, 1, "float64", None, True)
    _, U1 = guarded(eng1, pr["p"])
    alone = start_and_read(eng1, U1, Uh[:, :1], m[:, :1], v[:, :1])
    assert same_bits(alone, one[[0]])[0]
    # other neighbours, same bits
    m2, v2 = gc.rows(rng, k, M)
    m2[:, 64], v2[:, 64] = m[:, 0], v[:, 0]
    three = start_and_read(eng, U, Uh, m2, v2)
    assert same_bits(three[[64]], one[[0]])[0]


# ---- end to end: gp_mh(chains=, pca_tools=) ------------------------------------------------------------------------------

def host_chain(enka, prior, y, Gamma, pca, compounded, seed, steps):
    """MCMC.gp_mh on the host for pca_tools (ces/sample.py:17-119), restated with its margins: (samples (p, steps + 1),
    margin and phi(current) per step)."""
    from ces_amd import emulate
    state = np.random.get_state()
    np.random.seed(seed)
    scales = np.linalg.cholesky(np.cov(enka.Ustar))
    yc = y.reshape(-1, 1)

    def score(u):
        gm, gv = emulate.predict_gps(enka, u.reshape(1, -1), pca_tools=pca)
        yG = gm - yc
        Sigma = Gamma + gv
        phi = (yG * np.linalg.solve(2 * Sigma, yG)).sum() - prior.logpdf(u.flatten())
        if compounded:
            phi += .5 * np.log(np.linalg.eigvals(Sigma)).sum()
        return phi

    cur = enka.Ustar.mean(axis=1)
    phi_c = score(cur)
    out, margins, phis = [cur.flatten()], [], []
    for _ in range(steps):
        prop = cur + scales @ np.random.normal(0, 1, enka.p)
        phi_p = score(prop)
        lu = np.log(np.random.uniform())
        margins.append(phi_c - phi_p - lu)
        phis.append(phi_c)
        if lu < phi_c - phi_p:
            cur, phi_c = prop, phi_p
        out.append(cur)
    np.random.set_state(state)
    return np.array(out).T, np.array(margins), np.array(phis)


@pytest.mark.parametrize("compounded", [False, True])
def test_chains1_reproduces_the_host_chain(compounded):
    from ces_amd import sample
    man, a = load_gold()
    enka, prior = gold_problem(a), gold_prior(a)
    pca = dict(VD_k=a["prob_VD_k"], mG=a["prob_mG"])
    Gamma, steps, seed = a["prob_Gamma_dense"], 20, 3100 + int(compounded)
    kw = dict(pca_tools=pca, Gamma=Gamma, noise_compounded=compounded)

    def run(**extra):
        mc = sample.MCMC()
        mc.mute_bar = True
        mc.y_obs = a["prob_y"]
        np.random.seed(seed)
        mc.gp_mh(enka, steps, prior, **kw, **extra)
        return mc
    host = run()
    mine, margins, phis = host_chain(enka, prior, a["prob_y"], Gamma, pca, compounded, seed, steps)
    np.testing.assert_allclose(mine, host.samples, rtol=1e-12, atol=1e-12)       # the restatement IS the host chain
    d = run(chains=1, start="mean")
    assert d.samples.shape == host.samples.shape == (2, steps + 1)
    off = np.any(np.abs(d.samples - host.samples) > 1e-9 * np.maximum(1.0, np.abs(host.samples)), axis=0)
    if off.any():                      # a tie ends the comparison: the step before the first difference lay inside the band
        t = int(np.flatnonzero(off)[0]) - 1
        assert abs(margins[t]) <= sr.BAND * max(1.0, abs(phis[t])), (t, margins[t], phis[t])
    else:
        assert abs(d.accept - host.accept) < 1e-12
    assert 0.0 < host.accept < 1.0


def test_33_chains_run_and_keep_the_layout():
    from ces_amd import sample
    man, a = load_gold()
    enka = gold_problem(a)
    mc = sample.MCMC()
    mc.mute_bar = True
    mc.y_obs = a["prob_y"]
    mc.noise = "device"
    mc.trace_stride = 5
    mc.gp_mh(enka, 20, gold_prior(a), chains=33, pca_tools=dict(VD_k=a["prob_VD_k"], mG=a["prob_mG"]),
             Gamma=a["prob_Gamma_dense"], noise_compounded=True)
    assert mc.samples.shape == (2, 5, 33) and mc.accept_chains.shape == (33,)
    assert np.all(np.isfinite(mc.samples)) and 0.0 < mc.accept < 1.0
    assert abs(mc.accept - mc.accept_chains.mean()) < 1e-12


# ---- ABI states ----------------------------------------------------------------------------------------------------------

def test_abi_states(eng_mod):
    rng = np.random.default_rng(4)
    n, k, M = 7, 3, 5
    pr = gc.problem(rng, n, k, 1e2, "pca")
    eng = eng_mod.Engine(pr["p"], n, M, dtype="float64")
    with pytest.raises(eng_mod.CesxError) as ei:                      # no problem yet
        eng.gp_dense_set(pr["B"], pr["g0"], True)
    assert ei.value.code == eng_mod.ESTATE and "cesx_set_problem" in str(ei.value)
    with pytest.raises(eng_mod.CesxError) as ei:
        eng.mh_phi()
    assert ei.value.code == eng_mod.ESTATE and "start" in str(ei.value)
    eng.set_problem(pr["y"], pr["Gamma"], pr["mu"], pr["Sp"], pr["mu"])
    eng.mh_set_proposal(None, 0.3 * np.linalg.cholesky(pr["Sp"]))
    eng.gp_set(trivial_image(pr["p"], k))
    _, U = guarded(eng, pr["p"])
    Uh = gc.states(rng, pr, M)
    put(U, Uh)
    m, v = gc.rows(rng, k, M)
    md, vd = dev(eng, m), dev(eng, v)
    with pytest.raises(eng_mod.CesxError) as ei:                      # no descriptor
        eng.gp_start("dense", U, md, vd)
    assert ei.value.code == eng_mod.ESTATE and "cesx_gp_dense_set" in str(ei.value)
    eng.gp_dense_set(pr["B"], pr["g0"], True)
    want, bound, _, _ = gc.reference(pr, m, v, Uh, True)
    eng.gp_start("dense", U, md, vd)
    assert np.all(np.abs(eng.mh_phi() - want) <= bound)
    for B, text in ((np.zeros((n, 0)), "k must be"), (np.zeros((n, n + 1)), "k must be")):      # refused: the descriptor stays
        with pytest.raises(ValueError, match=text):                  # (CESX_EINVAL)
            eng.gp_dense_set(B, None, False)
    eng.gp_start("dense", U, md, vd)
    assert np.all(np.abs(eng.mh_phi() - want) <= bound)
    eng.gp_set(trivial_image(pr["p"], n))
    with pytest.raises(ValueError, match="n_gp"):                     # the emulator's n_gp must be k (CESX_EINVAL)
        eng.gp_start("dense", U, md, vd)
    eng.gp_set(trivial_image(pr["p"], k))
    # a NULL g0 is zero
    eng.gp_dense_set(pr["B"], None, False)
    pr0 = dict(pr, g0=np.zeros(n))
    w0, b0, _, _ = gc.reference(pr0, m, v, Uh, False)
    eng.gp_start("dense", U, md, vd)
    assert np.all(np.abs(eng.mh_phi() - w0) <= b0)
    # a second problem drops the descriptor (and the proposal); (the binding passes only a CHANGED problem on)
    eng.set_problem(pr["y"] + 1.0, pr["Gamma"], pr["mu"], pr["Sp"], pr["mu"])
    eng.mh_set_proposal(None, 0.3 * np.linalg.cholesky(pr["Sp"]))
    with pytest.raises(eng_mod.CesxError) as ei:
        eng.gp_start("dense", U, md, vd)
    assert ei.value.code == eng_mod.ESTATE and "cesx_gp_dense_set" in str(ei.value)
    # past the limit
    big = eng_mod.Engine(2, 129, 3)
    big.set_problem(np.zeros(129), np.eye(129), np.zeros(2), np.eye(2), np.zeros(2))
    with pytest.raises(ValueError, match="128"):                      # (CESX_EINVAL)
        big.gp_dense_set(np.eye(129)[:, :4], None, False)


def test_mh_phi_reads_the_other_modes(eng_mod):
    """cesx_mh_phi after gp_start('var') and after mh_start: the references of oracle/stage_ref.py at the project's fp64 bar."""
    rng = np.random.default_rng(12)
    p, n, M = 3, 6, 70
    y, gam = rng.standard_normal(n), 0.1 + 0.1 * rng.random(n)
    mu, Sp = 0.1 * rng.standard_normal(p), np.diag(0.5 + rng.random(p))
    eng = eng_mod.Engine(p, n, M, dtype="float64")
    eng.set_problem(y, np.diag(gam), mu, Sp, mu)
    eng.mh_set_proposal(None, 0.3 * np.linalg.cholesky(Sp))
    eng.gp_set(trivial_image(p, n))
    _, U = guarded(eng, p)
    _, G = guarded(eng, n)
    Uh = mu[:, None] + 0.5 * rng.standard_normal((p, M))
    put(U, Uh)
    mean, var = y[:, None] + 0.3 * rng.standard_normal((n, M)), 0.05 + 0.1 * rng.random((n, M))
    md, vd = dev(eng, mean), dev(eng, var)
    eng.gp_start("var", U, md, vd)
    want = sr.gp_phi("var", mean, var, y, np.diag(gam), Uh, mu, Sp)
    assert np.all(np.abs(eng.mh_phi() - want) <= 1e-9 * np.maximum(1.0, np.abs(want)))
    put(G, mean)
    eng.mh_start(U, G)
    want = sr.mh_phi(mean, y, 1.0 / gam, Uh, mu, 1.0 / np.diag(Sp))
    assert np.all(np.abs(eng.mh_phi() - want) <= 1e-9 * np.maximum(1.0, np.abs(want)))
