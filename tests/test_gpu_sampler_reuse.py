"""One Sample-stage engine through every change of update, on the device (tables and runner: tests/sampler_reuse_cases.py).

  1. a block on a REUSED engine equals the same block on a FRESH one as bytes -- U, phi, the per-chain counters, the step count
     and, for the adapt blocks, the multiplier and its history -- at every position of the generated sequences: the pair cover,
     the NaN polluters, abandoned work, the chain statistics between and inside the blocks;
  2. the fresh blocks are right: held to the features' own fp64 numpy chains at the features' own criteria;
  3. controls: a seed, a step index or one start state off by one are reported by the same comparator;
  4. one MCMC object through a sequence of model_mh / gp_mh calls against fresh objects resumed at the same point;
  5. the cross-family call-order table, cell by cell."""
import os
import sys

import numpy as np
import pytest
from scipy import stats

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adapt_cases as ac  # noqa: E402
import map_cases as mc_  # noqa: E402
import sampler_reuse_cases as sc  # noqa: E402
from gp_cases import random_gps  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng_mod():
    import torch
    from ces_amd import engine
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return engine


def _engine(eng_mod, E, dtype, seed=sc.SEED):
    e = sc.ENGINES[E]
    return eng_mod.Engine(e["p"], e["n"], e["J"], dtype=dtype, seed=seed)


_TWINS = {}


def _twin(eng_mod, E, dtype, item):
    """The block ``item`` on a freshly created engine (created for it, closed behind it); one run per module."""
    key = (E, dtype) + tuple(item)
    if key not in _TWINS:
        kind, prob, noise, variant = item
        eng = _engine(eng_mod, E, dtype)
        try:
            _TWINS[key] = sc.run_block(eng, sc.spec(E, kind, prob), noise, variant)
        finally:
            eng.close()
    return _TWINS[key]


def _run_sequence(eng_mod, E, dtype, seq, between=None):
    """``seq`` on ONE engine; returns the positions whose read-backs differ from their twins'."""
    eng = _engine(eng_mod, E, dtype)
    bad = []
    try:
        for i, item in enumerate(seq):
            kind, prob, noise, variant = item
            got = sc.run_block(eng, sc.spec(E, kind, prob), noise, variant)
            diff = sc.differences(got, _twin(eng_mod, E, dtype, item))
            if diff:
                tw = _twin(eng_mod, E, dtype, item)
                chains = sorted({int(j) for k in diff if k.endswith("U") and got[k].shape == tw[k].shape
                                 for j in np.nonzero(np.any(got[k] != tw[k], axis=0) | np.any(np.isnan(got[k]) != np.isnan(tw[k]), axis=0))[0]})
                bad.append((i, item, seq[i - 1] if i else None, diff, chains[:8], len(chains)))
            if between is not None:
                between(eng, i)
    finally:
        eng.close()
    return bad


def _cases(fn):
    return [(E, dt, x) for E in sorted(sc.ENGINES) for dt in sc.DTYPES for x in fn(E, dt)]


def _id(c):
    return "%s-%s-%s" % c


# ---- 1. reused equals fresh ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", _cases(sc.kinds_of), ids=_id)
def test_pair_cover(eng_mod, case):
    """Every ordered pair of block kinds as consecutive blocks on one engine (the part of the cover that starts with ``first``):
    each block equals its twin on a fresh engine as bytes."""
    E, dtype, first = case
    bad = _run_sequence(eng_mod, E, dtype, sc.pair_cover(E, dtype, first))
    assert not bad, "(position, block, the block before it, keys that differ, chains): %r" % (bad,)


@pytest.mark.parametrize("case", _cases(sc.polluters), ids=_id)
def test_nan_polluter(eng_mod, case):
    """A gradient block whose last step is handed NaN in every column of its forward output -- every chain rejects, and g of the
    proposal, a / b, the momenta, z and alpha hold NaN when the next block starts -- in front of every kind: the next block equals
    its twin, and so does the polluted block."""
    E, dtype, polluter = case
    for prob in (0, 1):
        tw = _twin(eng_mod, E, dtype, (polluter, prob, "device", "nan"))
        if sc.KINDS[polluter]["adapt"]:      # (the read-back in front of the poisoned step, the last behind the join)
            assert np.array_equal(tw["cnt"], tw["pre_cnt"]) and tw["U"].tobytes() == tw["pre_U"].tobytes()      # every chain rejected
            assert tw["phi"].tobytes() == tw["pre_phi"].tobytes() and tw["steps"][0] == tw["pre_steps"][0] + 1
            clean = _twin(eng_mod, E, dtype, (polluter, prob, "device", None))
            assert clean["pre_U"].tobytes() == tw["pre_U"].tobytes() and not np.array_equal(clean["cnt"], tw["cnt"])
            continue
        assert np.array_equal(tw["cnt"], tw["r3_cnt"]) and tw["U"].tobytes() == tw["r3_U"].tobytes()      # every chain rejected
        assert tw["phi"].tobytes() == tw["r3_phi"].tobytes() and tw["steps"][0] == tw["r3_steps"][0] + 1
        clean = _twin(eng_mod, E, dtype, (polluter, prob, "device", None))
        assert clean["r3_U"].tobytes() == tw["r3_U"].tobytes() and not np.array_equal(clean["cnt"], tw["cnt"])      # (the clean step moves chains)
    bad = _run_sequence(eng_mod, E, dtype, sc.nan_cover(E, dtype, polluter))
    assert not bad, "(position, block, the block before it, keys that differ, chains): %r" % (bad,)


@pytest.mark.parametrize("case", _cases(lambda E, dt: sc.ABANDON_FORMS), ids=_id)
def test_abandoned_work(eng_mod, case):
    """A block broken off -- a propose without its accept, a begin and one leap without the accept, an armed handle with one of
    three adaptation steps made and never read -- in front of every kind."""
    E, dtype, form = case
    bad = _run_sequence(eng_mod, E, dtype, sc.abandon_cover(E, dtype, form))
    assert not bad, "(position, block, the block before it, keys that differ, chains): %r" % (bad,)


_STATS = {}


def _fresh_stats(eng_mod, E, dtype, i):
    """Use ``i`` on a fresh engine WITHOUT the abandoned run in front: a read behind a run that was begun and never read is held
    to a run that never had one (a leak out of the unread run would otherwise reach both sides alike)."""
    key = (E, dtype, i)
    if key not in _STATS:
        eng = _engine(eng_mod, E, dtype)
        try:
            _STATS[key] = sc.stats_use(eng, E, i, abandoned=False)
        finally:
            eng.close()
    return _STATS[key]


@pytest.mark.parametrize("dtype", sc.DTYPES)
@pytest.mark.parametrize("E", sorted(sc.ENGINES))
def test_chain_statistics_between_and_inside_blocks(eng_mod, E, dtype):
    """chain_summary_*, chain_hist_* and chain_acf_* between the blocks and once in the middle of a block, N, bins, pairs, lags and
    followed chains changing from use to use, every third use behind a run that was begun and never read: each read equals a
    fresh engine's read of the same draws, and the blocks around them equal their twins."""
    kinds = sc.kinds_of(E, dtype)
    seq = [(k, t % 2, sc.NOISES[t % 2], None) for t, k in enumerate(kinds[::2] + kinds[1::4])]
    eng = _engine(eng_mod, E, dtype)
    bad, use = [], [0]

    def stats(where):
        i = use[0]
        use[0] += 1
        diff = sc.differences(sc.stats_use(eng, E, i), _fresh_stats(eng_mod, E, dtype, i))
        if diff:
            bad.append(("stats", i, where, diff))
    try:
        for t, item in enumerate(seq):
            kind, prob, noise, _ = item
            mid = (lambda U, t=t: stats("inside %d %s" % (t, seq[t][0]))) if t % 3 == 1 else None
            got = sc.run_block(eng, sc.spec(E, kind, prob), noise, None, mid=mid)
            diff = sc.differences(got, _twin(eng_mod, E, dtype, item))
            if diff:
                bad.append(("block", t, item, diff))
            stats("behind %d %s" % (t, kind))
    finally:
        eng.close()
    assert use[0] >= len(seq) + 3 and not bad, bad


# ---- 2. the fresh blocks against the features' numpy chains ------------------------------------------------------------------

@pytest.mark.parametrize("case", _cases(lambda E, dt: [k for k in sc.kinds_of(E, dt)
                                                       if any(sc.has_reference(E, k, nz, dt) for nz in sc.NOISES)]), ids=_id)
def test_fresh_blocks_against_numpy(eng_mod, case):
    """The twins are right, not merely repeatable: end state and counts against the feature's own fp64 numpy chain at the feature's
    own criterion -- tests/test_gpu_map_langevin.py, test_gpu_hmc.py, test_gpu_gp_langevin.py, test_gpu_lineal_langevin.py and
    test_gpu_lineal_hmc.py: states within 1e-9 (1 + |U|) on 0.999 of the chains and accept rates within 1e-12 (fp32: 1e-4, 0.97,
    0.01), accept rates inside (0.05, 0.999); test_gpu_adapt.py: no chain differing by ac.CAP, history and multiplier within 1e-9,
    behind the adaptation phase and behind the two steps that follow the join; test_gpu_gp_chain.py (the random
    walk on the emulator under the device noise): equal counters, states within 1e-9 (1 + |U|)."""
    E, dtype, kind = case
    d = sc.KINDS[kind]
    for prob in (0, 1):
        sp = sc.spec(E, kind, prob)
        noise = [nz for nz in sc.NOISES if sc.has_reference(E, kind, nz, dtype)][0]
        got = _twin(eng_mod, E, dtype, (kind, prob, noise, None))
        Ur, acc, ad = sc.reference(sp)
        total = sc.n_steps(kind)
        if d["adapt"]:
            n_diff = int(ac.differing(got["U_adapt"].astype(np.float64), Ur).sum())
            print("\n[reuse ref] %s %s %s p%d: differing %d multiplier %.9f ref %.9f" % (E, dtype, kind, prob, n_diff, got["multiplier"][0], ad["multiplier"]))
            assert n_diff == 0
            assert np.all(np.abs(got["history"] - ad["history"]) <= 1e-9 * (1 + np.abs(ad["history"])))
            assert abs(got["multiplier"][0] - ad["multiplier"]) <= 1e-9 * ad["multiplier"]
            # ... and the steps behind the join, at the scales re-formed from the multiplier
            n_end = int(ac.differing(got["U"].astype(np.float64), ad["U_end"]).sum())
            rate_d, rate_r = got["cnt"].sum() / (sc.POST_STEPS * sp["J"]), acc.sum() / (sc.POST_STEPS * sp["J"])
            print("[reuse ref] %s %s %s p%d: behind the join differing %d accept device %.6f numpy %.6f" % (E, dtype, kind, prob, n_end, rate_d, rate_r))
            assert n_end == 0 and abs(rate_d - rate_r) <= 1e-12 and 0.05 < rate_d < 0.999
            continue
        Ud = got["U"].astype(np.float64)
        if d["fam"] == "gp" and d["sampler"] == "rw":
            print("\n[reuse ref] %s %s %s p%d: accepted %d ref %d" % (E, dtype, kind, prob, got["cnt"].sum(), acc.sum()))
            assert np.array_equal(got["cnt"].astype(np.int64), acc)
            assert np.all(np.abs(Ud - Ur) <= 1e-9 * (1 + np.abs(Ur)))
            assert 0.05 < got["cnt"].sum() / (total * sp["J"]) < 0.999
            continue
        tol = 1e-9 if dtype == "float64" else 1e-4
        agree = np.all(np.abs(Ud - Ur) <= tol * (1 + np.abs(Ur)), axis=0)
        rate_d, rate_r = got["cnt"].sum() / (total * sp["J"]), acc.sum() / (total * sp["J"])
        print("\n[reuse ref] %s %s %s p%d: agree %.5f accept device %.6f numpy %.6f" % (E, dtype, kind, prob, agree.mean(), rate_d, rate_r))
        assert agree.mean() >= (0.999 if dtype == "float64" else 0.97), agree.mean()
        assert abs(rate_d - rate_r) <= (1e-12 if dtype == "float64" else 0.01)
        assert 0.05 < rate_d < 0.999                               # (a step that always or never moves compares nothing)


# ---- 3. controls ---------------------------------------------------------------------------------------------------------------------

def test_controls_are_reported_by_the_comparator(eng_mod):
    """Equality is not vacuous: a twin with its seed off by one, with its first step index off by one and with one start state
    moved by one ulp in one chain each differ from the twin under the comparator of the sequences; a repeat does not."""
    for E, dtype, kind in (("A", "float64", "rw"), ("B", "float32", "lin_hmc"), ("A", "float64", "gp_lv")):
        sp = sc.spec(E, kind, 0)
        tw = _twin(eng_mod, E, dtype, (kind, 0, "device", None))

        def run(seed=sc.SEED, **kw):
            eng = _engine(eng_mod, E, dtype, seed=seed)
            try:
                return sc.run_block(eng, sp, "device", None, **kw)
            finally:
                eng.close()
        assert sc.differences(tw, run()) == []
        assert sc.differences(tw, run(seed=sc.SEED + 1)), (E, kind, "seed")
        assert sc.differences(tw, run(first_step=sp["base"] + 1)), (E, kind, "step index")
        U0 = np.asarray(sp["U0"], dtype=np.float64).astype(dtype)
        U0[0, 77] = np.nextafter(U0[0, 77], np.asarray(np.inf, dtype=dtype))
        moved = run(U0=U0.astype(np.float64))
        diff = sc.differences(tw, moved)
        assert diff, (E, kind, "ulp")
        # and only in that chain
        for k in diff:
            if k.endswith("U"):
                cols = np.nonzero(np.any(tw[k] != moved[k], axis=0))[0]
                assert list(cols) == [77], (E, kind, k, cols)


# ---- 4. one MCMC object through a sequence of calls -------------------------------------------------------------------------------

M_CHAINS = 130


def _flat(prefix, v, out):
    if isinstance(v, dict):
        for k in sorted(v):
            _flat("%s.%s" % (prefix, k), v[k], out)
    elif v is None:
        out[prefix] = np.zeros(0)
    else:
        out[prefix] = np.asarray(v)
    return out


def _mcmc_models():
    """Factories: the reused object and every twin get instances of their own (a model remembers which engine holds its map)."""
    from ces_amd import utils
    rng = np.random.default_rng(31)
    A1 = rng.standard_normal((2, 2)) / np.sqrt(2) + np.eye(2)
    A2 = rng.standard_normal((2, 2)) / np.sqrt(2) - np.eye(2)
    b1, Al = 0.5 * rng.standard_normal(2), rng.uniform(0.2, 1.0, (2, 2)) / 2
    u_true = np.array([0.3, 0.2])
    mk = dict(elliptic=lambda: utils.elliptic(), banana=lambda: utils.banana(),
              lin1=lambda A=None: utils.lineal((A1 if A is None else A).copy(), b1.copy()).enable_gradient(leapfrog=True),
              lin2=lambda: utils.lineal(A2.copy(), 0).enable_gradient(leapfrog=True),
              log=lambda: utils.lineal_log(Al.copy()).enable_gradient(leapfrog=True))
    ys = dict(elliptic=np.asarray(utils.elliptic()(u_true), dtype=np.float64) + 0.01, banana=mc_.BANANA_Y,
              lin1=A1 @ u_true + b1 + 0.05, lin2=A2 @ u_true - 0.05, log=Al @ np.exp(u_true) + 0.02)
    return mk, ys, A1


def _mcmc_calls():
    """(what, model or None, steps, kwargs): about a dozen calls that change update, leapfrog, fused, adapt, the model, the
    emulator mode and the summaries; lin1 / lin2 alternate and lin1's A is edited in place before its last call."""
    Gd = np.diag([0.04, 0.09])
    Gf = np.array([[0.05, 0.02], [0.02, 0.08]])
    marg = dict(bins=8, bins2d=4, pairs=[(0, 1)], range=[[-3.0, 3.0], [-4.0, 4.0]])
    return [
        ("model", "elliptic", 10, dict(Gamma=0.1 ** 2 * np.eye(2))),
        ("model", "banana", 8, dict(Gamma="banana", update="langevin", fused=False)),
        ("gp", None, 9, dict()),
        ("model", "lin1", 8, dict(Gamma=Gd, update="hmc", leapfrog=3)),
        ("gp", None, 10, dict(Gamma=Gd, noise_compounded=True, update="langevin", adapt=4)),
        ("model", "lin2", 8, dict(Gamma=Gf, update="langevin")),
        ("model", "banana", 12, dict(Gamma="banana", update="hmc", leapfrog=2, fused=True, summary=True, burn=2, marginals=marg, autocorr=3)),
        ("model", "lin1", 8, dict(Gamma=Gd, update="langevin")),
        ("gp", None, 9, dict(Gamma=Gf, pca=True, sigma_form="dense")),
        ("gp", None, 10, dict(Gamma=Gf, pca=True, sigma_form="projected", noise_compounded=True, update="hmc", leapfrog=2,
                              summary=True, autocorr=dict(lags=2, chains=33))),
        ("model", "lin1*", 9, dict(Gamma=Gd, update="hmc", leapfrog=2, adapt=3)),
        ("model", "log", 8, dict(Gamma=Gf, update="langevin")),
        ("model", "elliptic", 11, dict(Gamma=0.1 ** 2 * np.eye(2), update="pCN", beta=0.2, summary=True, burn=1, marginals=dict(marg, bins=5))),
        ("model", "banana", 8, dict(Gamma="banana", update="langevin", fused=True)),
        ("gp", None, 8, dict(Gamma=Gd, update="pCN", fused=True)),
    ]


def test_one_mcmc_object_through_a_sequence_of_calls(eng_mod):
    """The production path: ONE MCMC object (noise='device', chains=130, p = n_obs = 2: one cached engine) through model_mh / gp_mh
    calls that change everything that can change.  The twin of call i is a fresh MCMC with the same seed whose ``samples`` and
    ``_mh_next_step`` are what the reused object held before the call (the exact resume of tests/test_gpu_adapt.py); the new part
    of ``samples``, ``accept``, ``accept_chains``, ``fused_launches``, ``adapt``, ``summary``, ``marginals`` and ``autocorr`` are equal
    as bytes, and a call without marginals= / autocorr= leaves neither attribute."""
    from ces_amd import calibrate, sample, utils
    mk, ys, A1 = _mcmc_models()
    enka_m = calibrate.enka(2, 2, 130)
    enka_m.Ustar = mc_.start_ensemble("banana", 130, np.random.default_rng(4))
    enka_g = random_gps(np.random.default_rng(77), 2, 2, sc.JT, sc.FAMILY)
    y_gp = enka_g.Gstar.mean(axis=1) + 0.05
    rng = np.random.default_rng(8)
    pca = dict(VD_k=np.linalg.qr(rng.standard_normal((2, 2)))[0] * np.array([0.8, 0.3]), mG=0.1 * rng.standard_normal(2))
    prior = stats.multivariate_normal(mean=[0.2, -0.1], cov=[[2.0, 0.6], [0.6, 3.0]])
    prior_pcn = stats.multivariate_normal(mean=[0.2, -0.1], cov=[[2.0, 0.0], [0.0, 3.0]])

    def new():
        s = sample.MCMC()
        s.mute_bar, s.noise, s.engine_dtype, s.seed = True, "device", "float64", 99
        return s

    def call(s, models, what, name, steps, kw, A_now):
        kw = dict(kw)
        pr = prior_pcn if kw.get("update") == "pCN" and what == "model" else prior
        if what == "gp":
            s.y_obs = y_gp
            if kw.pop("pca", False):
                kw["pca_tools"] = pca
            s.gp_mh(enka_g, steps, pr, delta=0.2, chains=M_CHAINS, **kw)
            return
        key = name.rstrip("*")
        if key not in models:
            models[key] = mk[key](A_now) if key == "lin1" and A_now is not None else mk[key]()
        model = models[key]
        s.y_obs = ys[key]
        Gamma = kw.pop("Gamma")
        Gamma = utils.banana().Gamma if isinstance(Gamma, str) else Gamma
        s.model_mh(model, steps, pr, enka_m, Gamma, delta=0.5, chains=M_CHAINS, **kw)

    s, models = new(), {}
    first_engine, bad, A_now = None, [], None
    for i, (what, name, steps, kw) in enumerate(_mcmc_calls()):
        if name == "lin1*":                                     # the reused object's model is edited IN PLACE: same object, new contents
            models["lin1"].A[0, 0] += 0.5
            A_now = models["lin1"].A.copy()
        before = None if not hasattr(s, "samples") else np.array(s.samples)
        nxt = getattr(s, "_mh_next_step", 0)
        call(s, models, what, name, steps, kw, None)
        if first_engine is None:
            first_engine = s._mh_eng
        assert s._mh_eng is first_engine, i
        tw = new()                                              # (enka_g is shared: emulate.device_image builds host arrays anew on
        if before is not None:                                  #  every call and the emulator remembers no engine; the models do)
            tw.samples, tw._mh_next_step = before.copy(), nxt
        call(tw, {}, what, name, steps, kw, A_now)
        n_old = 0 if before is None else before.shape[1]
        assert tw.samples.shape == s.samples.shape and s.samples.shape[1] > n_old
        a = dict(samples=s.samples[:, n_old:], accept=s.accept, accept_chains=s.accept_chains, fused_launches=s.fused_launches,
                 next_step=s._mh_next_step)
        b = dict(samples=tw.samples[:, n_old:], accept=tw.accept, accept_chains=tw.accept_chains, fused_launches=tw.fused_launches,
                 next_step=tw._mh_next_step)
        for attr in ("adapt", "marginals", "autocorr") + (("summary",) if kw.get("summary") else ()):
            asked = kw.get(attr) is not None
            assert hasattr(s, attr) == asked and hasattr(tw, attr) == asked, (i, attr)      # a call without it leaves no attribute
            if asked:
                a[attr], b[attr] = getattr(s, attr), getattr(tw, attr)
        diff = sc.differences(_flat("call", a, {}), _flat("call", b, {}))
        print("\n[reuse mcmc] call %d %s %s %s: accept %.4f fused launches %d%s" % (i, what, name, {k: v for k, v in kw.items() if k not in ("Gamma", "marginals")},
                                                                                   s.accept, s.fused_launches, " DIFFERS " + repr(diff) if diff else ""))
        if diff:
            bad.append((i, what, name, diff))
        assert tw._mh_eng is not s._mh_eng                      # engines are per object: the twin ran on memory of its own
        tw._mh_eng.close()
    s._mh_eng.close()
    assert not bad, bad


# ---- 5. the call-order table ---------------------------------------------------------------------------------------------------------

class _Handle:
    """An engine of shape A with everything installed that can be, brought into a row's state with chains running."""

    def __init__(self, eng_mod, eng):
        import torch
        from ces_amd import emulate, utils
        self.m, self.eng, self.torch = eng_mod, eng, torch
        self.gp = sc.spec("A", "gp_lv", 0)                  # a diagonal Gamma: every likelihood mode is legal
        self.gp2 = sc.spec("A", "gp_lv", 1)
        self.pj = sc.spec("A", "gp_proj_lv", 0)
        self.lin = sc.spec("A", "lin_lv", 0)["lin"]
        self.banana = utils.banana()
        self.lineal = utils.lineal(self.lin["A"], self.lin["b"]).enable_gradient(leapfrog=True)
        self.img = emulate.device_image(self.gp["gp"]["enka"], self.gp["gp"]["enka"].gpmodels)
        self.S = self.gp["S"]
        p, n, J = 2, 2, 130
        f64 = lambda *s: torch.empty(s, dtype=torch.float64, device=eng.device)      # noqa: E731
        self.rows = (f64(n, J), f64(n, J), f64(n, p, J), f64(n, p, J))
        self.jac = (f64(n, J), f64(n, p, J))
        self.Gm, self.Gl = eng.empty(n), eng.empty(n)
        self.U, self.X, self.X2 = eng.empty(p), eng.empty(p), eng.empty(p)

    # forward outputs at the states T
    def fwd(self, T):
        eng = self.eng
        eng.gp_predict_grad(T, out=self.rows)
        self.banana.jacobian_device(eng, T, out=self.jac)
        self.banana.forward_device(eng, T, out=self.Gm)
        self.lineal.forward_device(eng, T, out=self.Gl)

    def problem(self, sp):
        from ces_amd import emulate
        eng, g = self.eng, self.pj["gp"]
        other = self.gp2 if sp is self.gp else self.gp        # (Engine.set_problem leaves an unchanged problem alone: change it, so that
        eng.set_problem(other["y"], other["Gamma"], other["mu"], other["cov"], other["mu"])      #  the call below reaches cesx_set_problem)
        eng.set_problem(sp["y"], sp["Gamma"], sp["mu"], sp["cov"], sp["mu"])
        eng.gp_proj_set(*emulate.project_sigma(sp["Gamma"], g["B"], g["g0"], sp["y"]), True)

    def step(self, fam, k, armed=False):
        """One full step of family ``fam`` with step index k."""
        eng, U, X = self.eng, self.U, self.X
        if fam == "mh":
            eng.mh_propose(k, U, out=X)
            self.fwd(X)
            eng.mh_accept(k, U, X, self.Gm)
        elif fam == "gp":
            eng.mh_propose(k, U, out=X)
            self.fwd(X)
            eng.gp_accept("gamma_var", k, U, X, self.rows[0], self.rows[1])
        elif fam in ("gp_lv", "mh_lv", "proj") and armed:
            eng.mh_hmc_begin(k, U, out=X)
            self.fwd(X)
            eng.mh_hmc_accept(k, U, X, *self.jac)
        elif fam == "lin" and armed:
            eng.mh_hmc_lineal_begin(k, U, out=X)
            self.fwd(X)
            eng.mh_hmc_lineal_accept(k, U, X, self.Gl)
        elif fam == "gp_lv":
            eng.gp_langevin_propose(k, U, out=X)
            self.fwd(X)
            eng.gp_langevin_accept("gamma_var", k, U, X, *self.rows)
        elif fam == "proj":
            eng.gp_langevin_propose(k, U, out=X)
            self.fwd(X)
            eng.gp_langevin_accept("proj", k, U, X, *self.rows)
        elif fam == "mh_lv":
            eng.mh_langevin_propose(k, U, out=X)
            self.fwd(X)
            eng.mh_langevin_accept(k, U, X, *self.jac)
        else:
            eng.mh_langevin_lineal_propose(k, U, out=X)
            self.fwd(X)
            eng.mh_langevin_lineal_accept(k, U, X, self.Gl)

    def start(self, fam):
        eng, U = self.eng, self.U
        self.fwd(U)
        {"mh": lambda: eng.mh_start(U, self.Gm), "gp": lambda: eng.gp_start("gamma_var", U, self.rows[0], self.rows[1]),
         "gp_lv": lambda: eng.gp_langevin_start("gamma_var", U, *self.rows), "proj": lambda: eng.gp_langevin_start("proj", U, *self.rows),
         "mh_lv": lambda: eng.mh_langevin_start(U, *self.jac), "lin": lambda: eng.mh_langevin_lineal_start(U, self.Gl)}[fam]()

    def setup(self, row):
        """The handle in state ``row``: the problem, the proposal, the installs, the row's start, ONE step, then what the row
        leaves pending."""
        eng, r = self.eng, sc.ROWS[row]
        self.U.copy_(eng.to_device(self.gp["U0"], 2, "co_U"))
        self.X.copy_(self.U)
        self.X2.copy_(self.U)
        self.problem(self.gp)
        eng.gp_set(self.img)
        self.banana.ensure_installed(eng)
        self.next = 11
        if r["kind"] is None and row == "no_proposal":
            self.fwd(self.U)
            return
        if r["kind"] == "rw":
            eng.mh_set_proposal("pCN" if row.startswith("pcn") else None, self.S, 0.3)
        else:
            eng.mh_set_proposal("langevin", self.S)
            self.lineal.langevin_device(eng)
        fam = r["start"] or {"lineal_reinstalled": "lin", "after_set_problem": "mh_lv"}.get(row)
        if fam is None:
            self.fwd(self.U)
            return
        if r["armed"] and fam != "lin":
            eng.mh_adapt_set(3, 0.651, sc.GAIN, sc.KAPPA)
        self.start(fam)
        if r["armed"] and fam == "lin":
            eng.mh_adapt_set(3, 0.651, sc.GAIN, sc.KAPPA)
        for k in range(3 if r["done"] else 1):
            self.step(fam, 7 + k, armed=r["armed"])
        if r["pending"] == "lv":
            eng.mh_langevin_propose(self.next, self.U, out=self.X)
        elif r["pending"] == "lin_lv":
            eng.mh_langevin_lineal_propose(self.next, self.U, out=self.X)
        elif r["pending"] == "hmc":
            eng.mh_hmc_begin(self.next, self.U, out=self.X)
        elif r["pending"] == "lin_hmc":
            eng.mh_hmc_lineal_begin(self.next, self.U, out=self.X)
        if row == "lineal_set_behind_a_proposal":
            eng.mh_langevin_propose(self.next, self.U, out=self.X)
            self.lineal.langevin_device(eng)
        elif row == "lineal_reinstalled":
            self.lineal.langevin_device(eng)
        elif row == "after_set_problem":
            self.problem(self.gp2)
        self.fwd(self.X if r["pending"] else self.U)

    def snapshot(self):
        out = dict(U=self.U.cpu().numpy().copy())
        try:
            out["phi"] = self.eng.mh_phi()
            steps, _, per = self.eng.mh_stats(per_chain=True)
            out["cnt"], out["steps"] = per.copy(), np.array([steps])
        except self.m.CesxError as exc:
            assert exc.code == self.m.ESTATE
        return out

    def cont(self, row):
        """The next legitimate step of the row, and what it leaves."""
        eng, r, k = self.eng, sc.ROWS[row], self.next
        out = {}
        if r["pending"]:
            self.fwd(self.X)
            {"lv": lambda: eng.mh_langevin_accept(k, self.U, self.X, *self.jac),
             "lin_lv": lambda: eng.mh_langevin_lineal_accept(k, self.U, self.X, self.Gl),
             "hmc": lambda: eng.mh_hmc_accept(k, self.U, self.X, *self.jac),
             "lin_hmc": lambda: eng.mh_hmc_lineal_accept(k, self.U, self.X, self.Gl)}[r["pending"]]()
        elif r["done"]:
            pass
        elif r["start"]:
            self.step(r["start"], k, armed=r["armed"])
        elif row == "lineal_reinstalled":
            self.start("lin")
            self.step("lin", k)
        else:
            if r["kind"] is None:
                eng.mh_set_proposal(None, self.S)
            self.start("mh")
            self.step("mh", k)
        if r["armed"]:
            found = eng.mh_adapt_read()
            out.update(multiplier=np.array([found["multiplier"]]), history=found["history"])
        out.update(self.snapshot())
        return out

    def call(self, col):
        """``col`` with valid arguments of the right sizes; returns 'OK' or the refusal's name."""
        eng, U, X, X2, k = self.eng, self.U, self.X, self.X2, self.next
        m, v, dm, dv = self.rows
        G, DG = self.jac
        fn = {
            "cesx_mh_start": lambda: eng.mh_start(U, self.Gm),
            "cesx_mh_propose": lambda: eng.mh_propose(k, U, out=X2),
            "cesx_mh_accept": lambda: eng.mh_accept(k, U, X, self.Gm),
            "cesx_mh_run_map": lambda: eng.mh_run_map(k, 1, U),
            "cesx_gp_predict": lambda: eng.gp_predict(U),
            "cesx_gp_predict_grad": lambda: eng.gp_predict_grad(U),
            "cesx_gp_start": lambda: eng.gp_start("gamma_var", U, m, v),
            "cesx_gp_accept": lambda: eng.gp_accept("gamma_var", k, U, X, m, v),
            "cesx_gp_run": lambda: eng.gp_run("gamma_var", k, 1, U),
            "cesx_mh_langevin_start": lambda: eng.mh_langevin_start(U, G, DG),
            "cesx_mh_langevin_propose": lambda: eng.mh_langevin_propose(k, U, out=X2),
            "cesx_mh_langevin_accept": lambda: eng.mh_langevin_accept(k, U, X, G, DG),
            "cesx_mh_langevin_run_map": lambda: eng.mh_langevin_run_map(k, 1, U),
            "cesx_gp_langevin_start": lambda: eng.gp_langevin_start("gamma_var", U, m, v, dm, dv),
            "cesx_gp_langevin_propose": lambda: eng.gp_langevin_propose(k, U, out=X2),
            "cesx_gp_langevin_accept": lambda: eng.gp_langevin_accept("gamma_var", k, U, X, m, v, dm, dv),
            "cesx_gp_proj_langevin_start": lambda: eng.gp_langevin_start("proj", U, m, v, dm, dv),
            "cesx_gp_proj_langevin_accept": lambda: eng.gp_langevin_accept("proj", k, U, X, m, v, dm, dv),
            "cesx_mh_langevin_lineal_start": lambda: eng.mh_langevin_lineal_start(U, self.Gl),
            "cesx_mh_langevin_lineal_propose": lambda: eng.mh_langevin_lineal_propose(k, U, out=X2),
            "cesx_mh_langevin_lineal_accept": lambda: eng.mh_langevin_lineal_accept(k, U, X, self.Gl),
            "cesx_mh_hmc_begin": lambda: eng.mh_hmc_begin(k, U, out=X2),
            "cesx_mh_hmc_leap": lambda: eng.mh_hmc_leap(X, G, DG),
            "cesx_mh_hmc_accept": lambda: eng.mh_hmc_accept(k, U, X, G, DG),
            "cesx_gp_hmc_leap": lambda: eng.gp_hmc_leap("gamma_var", X, m, v, dm, dv),
            "cesx_gp_hmc_accept": lambda: eng.gp_hmc_accept("gamma_var", k, U, X, m, v, dm, dv),
            "cesx_gp_proj_hmc_leap": lambda: eng.gp_hmc_leap("proj", X, m, v, dm, dv),
            "cesx_gp_proj_hmc_accept": lambda: eng.gp_hmc_accept("proj", k, U, X, m, v, dm, dv),
            "cesx_mh_hmc_run_map": lambda: eng.mh_hmc_run_map(k, 1, 2, U),
            "cesx_mh_hmc_lineal_begin": lambda: eng.mh_hmc_lineal_begin(k, U, out=X2),
            "cesx_mh_hmc_lineal_leap": lambda: eng.mh_hmc_lineal_leap(X, self.Gl, X2),
            "cesx_mh_hmc_lineal_accept": lambda: eng.mh_hmc_lineal_accept(k, U, X, self.Gl),
        }[col]
        try:
            fn()
        except ValueError:
            return sc.EINVAL
        except self.m.CesxError as exc:
            return {self.m.ESTATE: sc.ESTATE, self.m.EINVAL: sc.EINVAL}.get(exc.code, "code %d" % exc.code)
        self.torch.cuda.synchronize()
        return sc.OK


def test_regression_random_walk_accept_under_a_langevin_proposal_without_a_start(eng_mod):
    """The narrowest sequence behind the one difference the table found: a problem, a Langevin proposal, no start.  The header
    refuses the random-walk calls under that kind with CESX_EINVAL, unconditionally; cesx_mh_accept and cesx_gp_accept looked at the
    missing start first and answered CESX_ESTATE (cesx_mh_start, cesx_mh_propose, cesx_mh_run_map, cesx_gp_start and cesx_gp_run
    answered CESX_EINVAL all along)."""
    eng = _engine(eng_mod, "A", "float64")
    try:
        h = _Handle(eng_mod, eng)
        h.problem(h.gp)
        eng.gp_set(h.img)
        h.banana.ensure_installed(eng)
        eng.mh_set_proposal("langevin", h.S)
        h.U.copy_(eng.to_device(h.gp["U0"], 2, "co_U"))
        h.X.copy_(h.U)
        h.next = 3
        h.fwd(h.U)
        for col in ("cesx_mh_accept", "cesx_gp_accept", "cesx_mh_start", "cesx_mh_propose", "cesx_mh_run_map", "cesx_gp_start", "cesx_gp_run"):
            assert h.call(col) == sc.EINVAL, col
        with pytest.raises(ValueError, match="CESX_MH_LANGEVIN"):
            eng.mh_accept(3, h.U, h.X, h.Gm)
    finally:
        eng.close()


@pytest.mark.parametrize("row", list(sc.ROWS))
def test_call_order(eng_mod, row):
    """Every cell of the row: the handle is brought into the row's state with chains running and the call is made with valid
    arguments.  A refusal answers the table's code, leaves U, cesx_mh_phi and cesx_mh_stats as they were, and the next legitimate
    step then gives the bytes of a run that never made the refused call (the only way g, the noise block and the momenta can be
    seen from outside); an OK cell is one of the steps of the sequences above and answers OK."""
    eng = _engine(eng_mod, "A", "float64")
    bad = []
    try:
        h = _Handle(eng_mod, eng)
        h.setup(row)
        ref = h.cont(row)
        h.setup(row)
        assert sc.differences(ref, h.cont(row)) == [], "the row's own continuation does not repeat"
        for col in sc.COLUMNS:
            want = sc.CALL_ORDER[row][col]
            h.setup(row)
            before = h.snapshot()
            got = h.call(col)
            if got != want:
                bad.append((col, "answered", got, "the table says", want))
                continue
            if want == sc.OK:
                continue
            if sc.differences(before, h.snapshot()):
                bad.append((col, "the refused call changed", sc.differences(before, h.snapshot())))
            diff = sc.differences(ref, h.cont(row))
            if diff:
                bad.append((col, "the next step differs behind the refused call", diff))
    finally:
        eng.close()
    assert not bad, bad
