"""Darcy chains on the adjoint launch, on the device: cesx_mh_langevin_* / cesx_mh_hmc_* under cesx_mh_grad_source(READY)
(ces_amd/csrc/kernels_darcy_chain.hip) and ``model_mh(chains=M, update='langevin' / 'hmc')`` on ``darcy.model`` after
``enable_gradient()``.

Stage tests hold ONE launch to fp64 from what it read -- the device's own G and d go into the numpy restatement of
tests/darcy_chain_cases.py, |dev - ref| <= c eps B with the constants derived there; g, which the ABI does not expose, is read
through the next proposal.  The end-to-end step is held to darcy_grad_cases.np_step (the host adjoint) on every one of the 130
chains: the accept decisions (tests/test_darcy_chain_host.py has checked every |margin| > 1e-6) and Q within the adjoint bound.
The worst ratios of a run are printed when the module's tests are over (NOTEBOOK.md records them).
"""
import os
import sys

import numpy as np
import pytest
from scipy import stats

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import darcy_chain_cases as cc  # noqa: E402
import darcy_grad_cases as gc  # noqa: E402

pytestmark = pytest.mark.gpu

WORST = {"phi": 0.0, "Q": 0.0, "Q32": 0.0, "e2e": 0.0}


@pytest.fixture(scope="module")
def eng_mod():
    import torch
    from ces_amd import engine
    assert torch.cuda.is_available(), "these tests need the MI355X"
    yield engine
    print("\n[darcy chain] worst |dev - ref| / (c eps B): phi %.3g, positions %.3g (fp32 engine, with the 2^-24 of the store: %.3g); "
          "worst |Q_dev - Q_np| / bound of the whole step: %.3g" % (WORST["phi"], WORST["Q"], WORST["Q32"], WORST["e2e"]))


def _t64(eng, a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=eng.device)


class _Stage:
    """One engine on a stage problem under READY, with the host copies a stage test compares against."""

    def __init__(self, eng_mod, sp, M, dtype, arm=None):
        self.sp, self.f, self.S, self.dtype = sp, sp["f"], np.array(sp["S"]), dtype
        self.n, self.p = self.f["n"], self.f["p"]
        self.eng = eng = eng_mod.Engine(self.p, self.n, M, dtype=dtype)
        eng.set_problem(sp["y"], sp["Gamma"], sp["mean"], sp["cov"], sp["mean"])
        eng.mh_set_proposal("langevin", self.S)
        sp["model"].ensure_installed(eng)
        eng.mh_grad_source("ready")
        if arm:
            eng.mh_adapt_set(arm, 0.651)
        self.store = 2.0 ** -24 if dtype == "float32" else 0.0

    def grad(self, X):
        """The adjoint launch at the device tensor X: (G, d) on the device and the score of those very values on the host."""
        G, phid, d = self.sp["model"].gradient_device(self.eng, X)
        Xh = self.eng.to_host(X)
        return G, d, Xh, cc.ready_score(self.f, self.S, Xh, G.cpu().numpy(), d.cpu().numpy())

    def check_phi(self, dev, s, cols, what):
        tol = cc.c_phi(self.n, self.p) * cc.EPS * s["Bphi"][cols]
        err = np.abs(dev[cols] - s["phi"][cols])
        if cols.size:
            WORST["phi"] = max(WORST["phi"], float(np.max(err / tol)))
        assert np.all(err <= tol), (what, float(np.max(err / tol)))

    def check_pos(self, dev, ref, B, what):
        tol = cc.c_q(self.p) * cc.EPS * B
        tol = tol + self.store * (np.abs(ref) + tol)
        err = np.abs(dev - ref)
        key = "Q32" if self.store else "Q"
        WORST[key] = max(WORST[key], float(np.max(err / tol)))
        assert np.all(err <= tol), (what, float(np.max(err / tol)))


def _mix(acc, sa, sb):
    """Column-wise: the score sa where acc, sb elsewhere."""
    return {k: np.where(acc if sa[k].ndim == 1 else acc[None, :], sa[k], sb[k]) for k in sa}


def _logu(st, margin, Bm, acc):
    """log u that accepts the chains of ``acc`` and rejects the others by 1/2 either way; the margin's own error is far below it."""
    assert np.all(np.isfinite(margin)) and np.all(cc.c_m(st.n, st.p) * cc.EPS * Bm < 0.25)
    return np.where(acc, margin - 0.5, margin + 0.5)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("pkind", ["diag", "dense"])
@pytest.mark.parametrize("gkind", ["diag", "dense"])
@pytest.mark.parametrize("shape", cc.STAGE_SHAPES, ids=lambda s: "K%d-p%d-n%d-M%d" % s)
def test_stages(eng_mod, shape, gkind, pkind, dtype):
    """start; propose + Langevin accept; begin + leap + leapfrog accept -- each launch against its restatement on what it read."""
    K, p, n, M = shape
    sp = cc.stage_problem(K, p, n, M, gkind, pkind, dtype)
    st = _Stage(eng_mod, sp, M, dtype)
    eng, S, xi = st.eng, st.S, np.array(sp["xi"])
    # -- start
    U = eng.to_device(np.array(sp["U0"]), p, "U").clone()
    G, d, Uh, sU = st.grad(U)
    assert np.array_equal(Uh, sp["U0"])
    eng.mh_langevin_start(U, G, d)
    phi0 = eng.mh_phi()
    every = np.arange(M)
    st.check_phi(phi0, sU, every, "start phi")
    # -- propose (g of the start through it), then the Langevin accept
    P = eng.mh_langevin_propose(0, U, xi=eng.to_device(xi[0], p, "xi"))
    Pref, r, BP, Br = cc.ready_begin(S, Uh, xi[0], sU)
    st.check_pos(eng.to_host(P), Pref, BP, "propose after start")
    GP, dP, Ph, sP = st.grad(P)
    margin, Bm = cc.ready_margin(sU, sP, xi[0], r, Br)
    acc = np.arange(M) % 2 == 0                           # the even chains accept, the odd ones reject
    logu = _logu(st, margin, Bm, acc)
    eng.mh_langevin_accept(0, U, P, GP, dP, logu=_t64(eng, logu))
    U1 = eng.to_host(U)
    assert np.array_equal(U1, np.where(acc[None, :], Ph, Uh))
    phi1 = eng.mh_phi()
    st.check_phi(phi1, sP, every[acc], "accepted phi")
    assert np.array_equal(phi1[~acc], phi0[~acc])
    steps, rate, per = eng.mh_stats(per_chain=True)
    assert steps == 1 and np.array_equal(per, acc.astype(np.uint64))
    s1 = _mix(acc, sP, sU)
    # -- begin (g after the accept through it: the accepted chains' is g(P), the others kept theirs), leap, leapfrog accept
    Q = eng.mh_hmc_begin(1, U, xi=eng.to_device(xi[1], p, "xi"))
    Qref, r, BQ, Br = cc.ready_begin(S, U1, xi[1], s1)
    st.check_pos(eng.to_host(Q), Qref, BQ, "begin after the Langevin accept")
    GQ, dQ, Q0h, sQ0 = st.grad(Q)
    eng.mh_hmc_leap(Q, GQ, dQ)
    Qref, r, BQ, Br = cc.ready_leap(S, Q0h, r, Br, sQ0)
    st.check_pos(eng.to_host(Q), Qref, BQ, "leap")
    GQ, dQ, Q1h, sQ1 = st.grad(Q)
    margin, Bm = cc.ready_margin(s1, sQ1, xi[1], r, Br)
    acc2 = ~acc if M > 1 else acc                         # (the other parity: every chain is accepted once and rejected once)
    logu = _logu(st, margin, Bm, acc2)
    eng.mh_hmc_accept(1, U, Q, GQ, dQ, logu=_t64(eng, logu))
    U2 = eng.to_host(U)
    assert np.array_equal(U2, np.where(acc2[None, :], Q1h, U1))
    phi2 = eng.mh_phi()
    st.check_phi(phi2, sQ1, every[acc2], "leapfrog accepted phi")
    assert np.array_equal(phi2[~acc2], phi1[~acc2])
    steps, rate, per = eng.mh_stats(per_chain=True)
    assert steps == 2 and np.array_equal(per, acc.astype(np.uint64) + acc2.astype(np.uint64))
    s2 = _mix(acc2, sQ1, s1)
    P = eng.mh_langevin_propose(2, U, xi=eng.to_device(xi[2], p, "xi"))
    Pref, r, BP, Br = cc.ready_begin(S, U2, xi[2], s2)
    st.check_pos(eng.to_host(P), Pref, BP, "propose after the leapfrog accept")
    eng.close()


def test_armed_steps_run_at_e_S(eng_mod):
    """Two steps of an armed handle at the first shape (leapfrog 1, then 2): the second runs at the multiplier the first step's
    recursion left, so e S, e g and alpha are under test at e != 1.  The history gives e_t and the pooled alpha of each step."""
    K, p, n, M = cc.STAGE_SHAPES[0]
    sp = cc.stage_problem(K, p, n, M, "dense", "dense", "float64")
    st = _Stage(eng_mod, sp, M, "float64", arm=2)
    eng, S, xi = st.eng, st.S, np.array(sp["xi"])
    U = eng.to_device(np.array(sp["U0"]), p, "U").clone()
    G, d, Uh, sU = st.grad(U)
    eng.mh_langevin_start(U, G, d)
    rec = []
    for t, L in ((0, 1), (1, 2)):
        Q = eng.mh_hmc_begin(t, U, xi=eng.to_device(xi[t], p, "xi"))
        pos = [eng.to_host(Q)]
        scores = []
        for _ in range(L - 1):
            GQ, dQ, Qh, sQ = st.grad(Q)
            scores.append(sQ)
            eng.mh_hmc_leap(Q, GQ, dQ)
            pos.append(eng.to_host(Q))
        GQ, dQ, Qh, sQ = st.grad(Q)
        scores.append(sQ)
        logu = np.full(M, -0.7)
        eng.mh_hmc_accept(t, U, Q, GQ, dQ, logu=_t64(eng, logu))
        rec.append(dict(L=L, pos=pos, scores=scores, U=eng.to_host(U), phi=eng.mh_phi()))
    found = eng.mh_adapt_read()
    hist = found["history"]
    assert found["steps"] == 2 and hist[0, 0] == 1.0 and hist[1, 0] != 1.0 and np.isfinite(found["multiplier"])
    Uc, sc_ = Uh, sU
    for t, row in enumerate(rec):
        e = float(hist[t, 0])
        Qref, r, BQ, Br = cc.ready_begin(S, Uc, xi[t], sc_, e)
        st.check_pos(row["pos"][0], Qref, BQ, "armed begin %d" % t)
        for k in range(row["L"] - 1):
            Qref, r, BQ, Br = cc.ready_leap(S, row["pos"][k], r, Br, row["scores"][k], e)
            st.check_pos(row["pos"][k + 1], Qref, BQ, "armed leap %d" % t)
        margin, Bm = cc.ready_margin(sc_, row["scores"][-1], xi[t], r, Br, e)
        tolm = cc.c_m(n, p) * cc.EPS * Bm
        assert np.all(np.abs(margin + 0.7) > 1e-6), "a chain's test is within rounding of log u: change log u"
        acc = margin > -0.7
        assert np.array_equal(row["U"], np.where(acc[None, :], row["pos"][-1], Uc))
        abar = float(np.mean(cc.alpha_of(margin)))
        assert abs(hist[t, 1] - abar) <= float(np.mean(tolm)) + M * cc.EPS, (t, hist[t, 1], abar)
        st.check_phi(row["phi"], row["scores"][-1], np.arange(M)[acc], "armed phi %d" % t)
        Uc, sc_ = row["U"], _mix(acc, row["scores"][-1], sc_)
    eng.close()


# ---- the whole step against the host adjoint -----------------------------------------------------------------------------------

def _mcmc(gkind="diag", noise="device", seed=77, dtype="float64", trunc=False):
    from ces_amd import calibrate, sample
    prob = gc.step_problem(gkind)
    K, p, n = gc.STEP_SHAPE
    enka = calibrate.enka(p, n, gc.M_STEP)
    enka.Ustar = np.array(prob["Ustar"])
    s = sample.MCMC()
    s.mute_bar, s.y_obs, s.noise, s.seed, s.engine_dtype = True, prob["y"], noise, seed, dtype
    return s, enka, stats.multivariate_normal(mean=prob["mean"], cov=prob["cov"]), prob


@pytest.mark.parametrize("L", [1, 3])
@pytest.mark.parametrize("gkind", ["diag", "dense"])
def test_one_step_is_np_step_on_every_chain(eng_mod, gkind, L):
    """Ustar, injected xi and log u, the engine driven as ``bind_langevin_darcy`` / ``bind_hmc_darcy`` drive it: U_next equals
    gc.np_step's on all 130 chains (every decision, and Q within the adjoint bound carried through the step plus the stage bound)."""
    ref = cc.step_reference(gkind, L)
    prob, S = ref["prob"], np.array(ref["S"])
    K, p, n = gc.STEP_SHAPE
    M = gc.M_STEP
    sp = dict(model=prob["model"], y=prob["y"], Gamma=prob["Gamma"], mean=prob["mean"], cov=prob["cov"], S=S, f=cc.factors(prob))
    st = _Stage(eng_mod, sp, M, "float64")
    eng = st.eng
    U = eng.to_device(np.array(ref["U"]), p, "U").clone()
    G, d, Uh, sU = st.grad(U)
    eng.mh_langevin_start(U, G, d)
    xi_t, logu_t = eng.to_device(np.array(ref["xi"]), p, "xi"), _t64(eng, np.array(ref["logu"]))
    if L == 1:
        Q = eng.mh_langevin_propose(0, U, xi=xi_t)
        Qref, r, BQ, Br = cc.ready_begin(S, Uh, np.array(ref["xi"]), sU)
        GQ, dQ, Qh, sQ = st.grad(Q)
        eng.mh_langevin_accept(0, U, Q, GQ, dQ, logu=logu_t)
    else:
        Q = eng.mh_hmc_begin(0, U, xi=xi_t)
        Qref, r, BQ, Br = cc.ready_begin(S, Uh, np.array(ref["xi"]), sU)
        for _ in range(L - 1):
            GQ, dQ, Qh, sQ = st.grad(Q)
            eng.mh_hmc_leap(Q, GQ, dQ)
            Qref, r, BQ, Br = cc.ready_leap(S, Qh, r, Br, sQ)
        GQ, dQ, Qh, sQ = st.grad(Q)
        eng.mh_hmc_accept(0, U, Q, GQ, dQ, logu=logu_t)
    Un = eng.to_host(U)
    stage = L * cc.c_q(p) * cc.EPS * BQ                   # (the stage bound of each of the L positions, the last one's B the largest)
    tol = ref["bound"] + stage
    err = np.abs(Qh - ref["Q"])
    WORST["e2e"] = max(WORST["e2e"], float(np.max(err / tol)))
    print("%s L=%d: worst |Q_dev - Q_np| / bound %.3g" % (gkind, L, float(np.max(err / tol))))
    assert np.all(err <= tol), float(np.max(err / tol))
    assert np.array_equal(Un, np.where(ref["acc"][None, :], Qh, Uh))
    steps, rate, per = eng.mh_stats(per_chain=True)
    assert np.array_equal(per.astype(bool), ref["acc"])
    assert np.max(np.abs(Un - ref["U_next"])) <= float(np.max(tol))
    eng.close()


# ---- model_mh itself -------------------------------------------------------------------------------------------------------------

def _run(update, n_mcmc=20, delta=None, leapfrog=None, seed=77, sampler=None, **kw):
    s, enka, prior, prob = _mcmc(seed=seed)
    s = sampler or s
    for k in ("samples", "_mh_next_step"):
        s.__dict__.pop(k, None)
    if leapfrog is not None:
        kw["leapfrog"] = leapfrog
    delta = cc.STEP_DELTA if delta is None else delta
    if update is not None:
        kw["update"] = update
    s.model_mh(prob["model"], n_mcmc, prior, enka, prob["Gamma"], delta=delta, chains=gc.M_STEP, start="ensemble", **kw)
    return s


def test_model_mh_langevin_and_hmc(eng_mod):
    """20 steps, device noise, twice from one seed: bit-identical; leapfrog=1 is 'langevin' bit for bit; summary=True runs.  The
    accept rates at the delta of the host test (tests/test_darcy_chain_host.py holds np_step's decisions at cc.STEP_DELTA = 1.8, the
    step of tests/test_darcy_grad_host.py's leapfrog chain) lie in (0.05, 0.99): measured 0.7554 (Langevin) and 0.7885 (leapfrog 3).
    (At delta = 0.3, the step of the host Langevin chain of tests/test_darcy_grad_host.py, 130 Langevin chains accept 0.9988 of
    2 600 proposals -- np_step accepts 129 or 130 of 130 there as well: a step that small is hardly ever refused.)"""
    a, b = _run("langevin"), _run("langevin")
    assert a.samples.shape == (gc.STEP_SHAPE[1], 21, gc.M_STEP) and np.all(np.isfinite(a.samples))
    assert np.array_equal(a.samples, b.samples) and a.accept == b.accept and np.array_equal(a.accept_chains, b.accept_chains)
    one = _run("hmc", leapfrog=1)
    assert np.array_equal(a.samples, one.samples) and a.accept == one.accept
    h, h2 = _run("hmc", leapfrog=3), _run("hmc", leapfrog=3)
    assert np.array_equal(h.samples, h2.samples) and h.accept == h2.accept
    assert not np.array_equal(h.samples, a.samples)
    print("[darcy chain] accept at delta %.1f: langevin %.4f, hmc L=3 %.4f" % (cc.STEP_DELTA, a.accept, h.accept))
    assert 0.05 < a.accept < 0.99 and 0.05 < h.accept < 0.99
    sm = _run("hmc", leapfrog=3, summary=True)
    assert sm.summary["n"] == 20 and np.all(np.isfinite(sm.summary["mean"]))
    assert np.array_equal(sm.samples[:, -1, :], h.samples[:, -1, :])


def test_model_mh_adapt_joins_exactly(eng_mod):
    """adapt=20 of 30 steps ends with a finite multiplier, and a fresh sampler resumed from step 20 at delta' continues bit for bit."""
    X = _run("hmc", n_mcmc=30, leapfrog=3, adapt=20)
    assert np.isfinite(X.adapt["multiplier"]) and X.adapt["multiplier"] > 0 and X.adapt["steps"] == 20
    s, enka, prior, prob = _mcmc()
    s.samples, s._mh_next_step = X.samples[:, :21, :].copy(), 20
    s.model_mh(prob["model"], 10, prior, enka, prob["Gamma"], delta=X.adapt["delta"], chains=gc.M_STEP, start="ensemble",
               update="hmc", leapfrog=3)
    assert np.array_equal(s.samples, X.samples)
    lv = _run("langevin", n_mcmc=24, adapt=20)
    assert np.isfinite(lv.adapt["multiplier"]) and np.all(np.isfinite(lv.samples))


def test_model_trunc_and_float32_run(eng_mod):
    """``model_trunc`` (the step problem's own model) for 5 steps on an fp32 engine, and ``darcy.model`` (p = K^2) on an fp64 one."""
    from ces_amd import calibrate, darcy, sample
    s, enka, prior, prob = _mcmc(dtype="float32")
    assert isinstance(prob["model"], darcy.model_trunc)
    s.model_mh(prob["model"], 5, prior, enka, prob["Gamma"], delta=0.3, chains=gc.M_STEP, start="ensemble", update="langevin")
    assert s.samples.shape[1] == 6 and np.all(np.isfinite(s.samples)) and 0 < s.accept <= 1
    mdl = darcy.model(Nmesh=4.0)
    mdl.obs_index = np.array([5, 10, 3])
    mdl.enable_gradient()
    rng = np.random.default_rng(3)
    truth = 0.5 * rng.standard_normal(16)
    y = mdl(truth)
    Gam = gc.gamma("dense", 3, 0.05 * float(np.max(np.abs(y))))
    enka = calibrate.enka(16, 3, 40)
    enka.Ustar = truth[:, None] + 0.3 * rng.standard_normal((16, 40))
    s = sample.MCMC()
    s.mute_bar, s.y_obs, s.noise = True, y, "device"
    s.model_mh(mdl, 5, stats.multivariate_normal(mean=np.zeros(16), cov=np.eye(16)), enka, Gam, delta=0.3, chains=7,
               start="ensemble", update="hmc", leapfrog=2)
    assert s.samples.shape == (16, 6, 7) and np.all(np.isfinite(s.samples))


# ---- failed particles ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("L", [1, 3])
def test_a_failed_position_is_rejected_alone(eng_mod, L):
    """One chain's injected xi carries an entry that takes exp(theta) out of fp64 at the first position (the construction of
    test_gpu_darcy_grad's overflowing particle): G, phi_d and d are NaN there, the chain keeps U, phi, g and its counter bit
    for bit, and every other chain equals a run without the entry.  At L = 3 the leap kernel meets the failed position."""
    ref = cc.step_reference("diag", L)
    prob, S = ref["prob"], np.array(ref["S"])
    K, p, n = gc.STEP_SHAPE
    M, bad = gc.M_STEP, 5
    sp = dict(model=prob["model"], y=prob["y"], Gamma=prob["Gamma"], mean=prob["mean"], cov=prob["cov"], S=S, f=cc.factors(prob))
    runs = []
    for poisoned in (False, True):
        st = _Stage(eng_mod, sp, M, "float64")
        eng = st.eng
        U = eng.to_device(np.array(ref["U"]), p, "U").clone()
        G, d, Uh, sU = st.grad(U)
        eng.mh_langevin_start(U, G, d)
        phi0 = eng.mh_phi()
        xi = np.array(ref["xi"])
        if poisoned:
            xi[:, bad] = 1e8
        logu_t = _t64(eng, np.array(ref["logu"]))
        Q = eng.mh_hmc_begin(0, U, xi=eng.to_device(xi, p, "xi"))
        for _ in range(L - 1):
            GQ, dQ, Qh, sQ = st.grad(Q)
            eng.mh_hmc_leap(Q, GQ, dQ)
        GQ, dQ, Qh, sQ = st.grad(Q)
        if poisoned:
            assert np.all(np.isnan(GQ.cpu().numpy()[:, bad])) and np.all(np.isnan(dQ.cpu().numpy()[:, bad]))
        eng.mh_hmc_accept(0, U, Q, GQ, dQ, logu=logu_t)
        Un, phi1 = eng.to_host(U), eng.mh_phi()
        steps, rate, per = eng.mh_stats(per_chain=True)
        nxt = eng.to_host(eng.mh_langevin_propose(1, U, xi=eng.to_device(np.array(ref["xi"]), p, "xi")))      # (g through it)
        runs.append(dict(U=Un, phi=phi1, per=per, nxt=nxt, U0=Uh, phi0=phi0))
        eng.close()
    clean, pois = runs
    good = np.arange(M) != bad
    for k in ("U", "phi", "per", "nxt"):
        assert np.array_equal(clean[k][..., good], pois[k][..., good]), k
    assert np.array_equal(pois["U"][:, bad], pois["U0"][:, bad]) and pois["phi"][bad] == pois["phi0"][bad] and pois["per"][bad] == 0
    assert np.all(np.isfinite(pois["nxt"][:, bad]))
    # the chain's g is the start's: its next proposal is the one a chain that never moved would make
    if not clean["per"][bad]:
        assert np.array_equal(pois["nxt"][:, bad], clean["nxt"][:, bad])


def test_a_failing_start_state_raises(eng_mod):
    s, enka, prior, prob = _mcmc()
    Ustar = np.array(prob["Ustar"])
    Ustar[:, 3] = 1e5
    enka.Ustar = Ustar
    with pytest.raises(ValueError, match="start state of chain 3"):
        s.model_mh(prob["model"], 4, prior, enka, prob["Gamma"], delta=0.3, chains=gc.M_STEP, start="ensemble", update="langevin",
                   enka_scaling=False)
    assert not hasattr(s, "samples")


# ---- reuse -----------------------------------------------------------------------------------------------------------------------

def test_one_engine_across_updates_equals_fresh_engines(eng_mod):
    """rw, langevin, hmc, adapt, rw on ONE sampler (one engine) against a fresh sampler per leg: bit-identical legs."""
    legs = [dict(update=None, delta=0.3), dict(update="langevin"), dict(update="hmc", leapfrog=3),
            dict(update="hmc", leapfrog=2, adapt=4, delta=1.0), dict(update=None, delta=0.3)]
    shared, _, _, _ = _mcmc()
    engines = set()
    for leg in legs:
        kw = dict(leg)
        one = _run(kw.pop("update"), n_mcmc=6, sampler=shared, **kw)
        engines.add(id(shared._mh_eng))
        got = (one.samples.copy(), one.accept, one.accept_chains.copy())
        kw = dict(leg)
        fresh = _run(kw.pop("update"), n_mcmc=6, **kw)
        assert np.array_equal(got[0], fresh.samples) and got[1] == fresh.accept and np.array_equal(got[2], fresh.accept_chains), leg
    assert len(engines) == 1


def test_the_source_returns_to_the_jacobian_image(eng_mod):
    """ESTATE before a proposal, EINVAL for an unknown source; after READY a cesx_mh_set_proposal (and a cesx_set_problem) puts the
    Jacobian image back: the start on [n][p][J] inputs gives the bits of an engine that never heard of the call."""
    import torch
    E = eng_mod
    K, p, n = gc.STEP_SHAPE
    prob = gc.step_problem("dense")
    M = 9
    S = cc.step_scale(prob, 0.3)
    rng = np.random.default_rng(1)
    Uh = np.array(prob["Ustar"][:, :M])
    Gh, DGh, xih = rng.standard_normal((n, M)), rng.standard_normal((n, p, M)), rng.standard_normal((p, M))

    def start_and_propose(eng):
        U = eng.to_device(Uh, p, "U").clone()
        eng.mh_langevin_start(U, _t64(eng, Gh), _t64(eng, DGh))
        return eng.mh_phi(), eng.to_host(eng.mh_langevin_propose(0, U, xi=eng.to_device(xih, p, "xi")))

    a = E.Engine(p, n, M, dtype="float64")
    assert a.lib.cesx_mh_grad_source(a._h, 1) == E.ESTATE
    a.set_problem(prob["y"], prob["Gamma"], prob["mean"], prob["cov"], prob["mean"])
    assert a.lib.cesx_mh_grad_source(a._h, 1) == E.ESTATE
    a.mh_set_proposal(None, S)
    assert a.lib.cesx_mh_grad_source(a._h, 1) == E.ESTATE                   # (a random-walk proposal)
    a.mh_set_proposal("langevin", S)
    assert a.lib.cesx_mh_grad_source(a._h, 2) == E.EINVAL and a.lib.cesx_mh_grad_source(a._h, -1) == E.EINVAL
    with pytest.raises(ValueError):
        a.mh_grad_source("image")
    a.mh_grad_source("ready")
    prob["model"].ensure_installed(a)
    U = a.to_device(Uh, p, "U").clone()
    G, phid, d = prob["model"].gradient_device(a, U)
    a.mh_langevin_start(U, G, d)
    ready_phi = a.mh_phi()
    a.mh_set_proposal("langevin", S)                      # the source is the Jacobian image again
    phi_a, P_a = start_and_propose(a)
    b = E.Engine(p, n, M, dtype="float64")
    b.set_problem(prob["y"], prob["Gamma"], prob["mean"], prob["cov"], prob["mean"])
    b.mh_set_proposal("langevin", S)
    phi_b, P_b = start_and_propose(b)
    assert np.array_equal(phi_a, phi_b) and np.array_equal(P_a, P_b) and not np.array_equal(phi_a, ready_phi)
    a.mh_grad_source("ready")
    a.mh_grad_source("jacobian")                          # and the call itself switches back
    phi_c, P_c = start_and_propose(a)
    assert np.array_equal(phi_c, phi_b) and np.array_equal(P_c, P_b)
    assert torch.cuda.is_available()
    a.close()
    b.close()
