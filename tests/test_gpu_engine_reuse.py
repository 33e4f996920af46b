"""The sequences of tests/reuse_cases.py on a device: ONE ``ces_amd.engine.Engine`` driven through a list of steps, every step
held to fp64 of its own inputs (checks 1-5 of reuse_cases.py, its bars unchanged).

R   the rules on one problem, on E1 / E2 / E3 under the call flows step, split, sharded and cycle, both problem families;
    the same through ShardedUpdate pipelined against plain, bit for bit, warm and with CESX_NS_WARM=0
P   six problems on one engine with a ``chain`` flip off and on again
S   the Sample stage on the engine between steps 4 and 5 (``mh_case`` at the engine's own shape, RW and pCN, ``mh_propose``,
    on fp64 the installed linear map), then the problem set again: the proposal is gone and the remaining steps hold
T   every other stage between steps that leave the problem alone, in ``between`` and behind the launch of the step before
    (``before_result``); each block call must return what the same calls return on a fresh engine, BIT FOR BIT: the kernels,
    tables, inputs and Philox words are the same and the suite holds these kernels to be reproducible and placement free
the drop-in object: one ``ces_amd.calibrate.sampling`` object through R's rule list against one carried ``OracleState``

When the module ends it prints one ENGINE-REUSE line per part: the worst ratio to a bar, the comparisons, the (form,
warm_inverse) log of every sequence."""
import os
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import darcy_cases as dc  # noqa: E402
import darcy_stream_cases as dsc  # noqa: E402
import gp_cases as gc  # noqa: E402
import l96_cases as lc  # noqa: E402
import reuse_cases as rc  # noqa: E402
import test_gpu_sample_edges as se  # noqa: E402
from edge_helpers import guarded, guards_intact  # noqa: E402

from oracle import calibrate_ref as cr  # noqa: E402
from oracle import ces_numpy as oc  # noqa: E402
from oracle import stage_ref as sr  # noqa: E402

pytestmark = pytest.mark.gpu

PARTS = ("R", "R pipelined", "P", "S", "T", "drop-in")
RECS = {part: rc.Record() for part in PARTS}
LOGS = {part: [] for part in PARTS}


@pytest.fixture(scope="module")
def eng_mod():
    import torch
    from ces_amd import build, engine
    build.build_lib()
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return engine


@pytest.fixture(scope="module", autouse=True)
def the_record():
    yield
    for part in PARTS:
        rec = RECS[part]
        if not rec.rows:
            continue
        worst = max(rec.worst.items(), key=lambda kv: kv[1][0])
        print("\nENGINE-REUSE %-11s worst ratio to a bar %.3g (%s), %d comparisons; %s"
              % (part, worst[1][0], worst[0], len(rec.rows),
                 "; ".join("%s: %s" % (lab, " ".join("(%d,%d)" % fw for fw in log)) for lab, log in LOGS[part])))


def make_engine(eng_mod, shape):
    p, n, J, dtype = shape
    return eng_mod.Engine(p, n, J, dtype=dtype, seed=rc.SEED)


def forms_of(name, steps, probs):
    return [rc.expected_form(name, s, probs[s["prob"]]) for s in steps]


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- R ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fam", cr.FAMILIES)
@pytest.mark.parametrize("flow", rc.FLOWS + ("cycle",))
@pytest.mark.parametrize("name", sorted(rc.ENGINES))
def test_sequence_r(eng_mod, name, flow, fam):
    p, n, J, dtype = rc.ENGINES[name]
    A, U0, probs = rc.problems(fam, p, n, J, dtype)
    forms = forms_of(name, rc.R_STEPS, probs)
    eng = make_engine(eng_mod, rc.ENGINES[name])
    label = "R %s %s %s" % (name, fam, flow)
    log = rc.run_sequence(eng_mod, eng, A, U0, probs, rc.R_STEPS, flow, RECS["R"], label, forms=forms)
    LOGS["R"].append((label, log))
    assert [f for f, _ in log] == forms
    seen = {f for f, _ in log} - {-1}
    assert seen == {"E1": {2, 0}, "E2": {1, 0}, "E3": {0}}[name], seen
    eng.close()


@pytest.mark.parametrize("warm", [True, False], ids=["warm", "CESX_NS_WARM=0"])
@pytest.mark.parametrize("name", ["E1", "E3"])
def test_sequence_r_pipelined_equals_plain_bit_for_bit(eng_mod, monkeypatch, name, warm):
    """finish(i), begin(i + 1), result(i) against result(i) first: U_next and the seven scalars of every step, bit for bit."""
    if not warm:
        monkeypatch.setenv("CESX_NS_WARM", "0")               # read in cesx_create
    p, n, J, dtype = rc.ENGINES[name]
    A, U0, probs = rc.problems("data", p, n, J, dtype)
    rows = []
    for pipelined in (False, True):
        eng = make_engine(eng_mod, rc.ENGINES[name])
        label = "R %s data %s%s" % (name, "pipelined" if pipelined else "plain", "" if warm else " cold")
        rows.append(rc.run_pipelined(eng_mod, eng, A, U0, probs, rc.R_STEPS, RECS["R pipelined"], label, pipelined))
        eng.close()
    for i, ((ua, ra), (ub, rb)) in enumerate(zip(*rows)):
        RECS["R pipelined"].add("R %s bits" % name, i, "pipelined == plain", 0.0 if same_bytes(ua, ub) and same_bytes(ra, rb) else np.inf,
                                True, (name, warm, "step %d" % i, "U_next equal: %s" % same_bytes(ua, ub), ra, rb))


# ---- P ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fam", cr.FAMILIES)
@pytest.mark.parametrize("name", ["E1", "E3"])
def test_sequence_p(eng_mod, name, fam):
    p, n, J, dtype = rc.ENGINES[name]
    A, U0, probs = rc.problems(fam, p, n, J, dtype, "P")
    forms = forms_of(name, rc.P_STEPS, probs)
    if name == "E1":                                         # chain off (P1's dense Sigma) and on again
        chain = [f == 2 for f, s in zip(forms, rc.P_STEPS) if s["update"] == "aldi"][::2]
        assert sum(a != b for a, b in zip(chain, chain[1:])) == 2, forms
    eng = make_engine(eng_mod, rc.ENGINES[name])
    label = "P %s %s" % (name, fam)
    log = rc.run_sequence(eng_mod, eng, A, U0, probs, rc.P_STEPS, "cycle", RECS["P"], label, forms=forms)
    LOGS["P"].append((label, log))
    assert [f for f, _ in log] == forms
    eng.close()


# ---- S ------------------------------------------------------------------------------------------------------------------------

S_MH_STEP = 7


@pytest.mark.parametrize("fam", cr.FAMILIES)
@pytest.mark.parametrize("name", ["E1", "E3"])
def test_sequence_s(eng_mod, name, fam):
    import torch
    shape = rc.ENGINES[name]
    p, n, J, dtype = shape
    ndt = np.dtype(dtype)
    A, U0, probs = rc.problems(fam, p, n, J, dtype, "S")
    forms = forms_of(name, rc.S_STEPS, probs)
    eng = make_engine(eng_mod, shape)
    rec, label = RECS["S"], "S %s %s" % (name, fam)
    rng = np.random.default_rng([rc.SEED, p, n, J, 5])
    Xh = (probs[0]["mu"] + 0.5 * rng.standard_normal((p, J))).astype(ndt)
    Bs = rng.standard_normal((p, p)) / np.sqrt(p)
    S = np.linalg.cholesky(0.5 * (Bs @ Bs.T) + 0.5 * np.eye(p))
    Al, bl = (rng.standard_normal((n, p)) / np.sqrt(p)).astype(ndt), rng.standard_normal(n).astype(ndt)
    X = torch.as_tensor(Xh, device=eng.device)
    state = {}

    def block(e):
        assert e is eng
        shared = types.SimpleNamespace(Engine=lambda *a, **k: eng)
        for kind in (None, "pCN"):
            ref = se.mh_case(shared, dtype, p, n, J, kind, part="S on a reused engine")
            assert ref.left_out == 0 and ref.chain_steps == se.STEPS * J, (label, kind, ref.left_out)
        eng.mh_set_proposal(None, S)
        P_flat, P = guarded(eng, p)
        eng.mh_propose(S_MH_STEP, X, out=P)
        want = sr.propose(Xh.astype(np.float64), S, sr.mh_noise(p, J, rc.SEED, S_MH_STEP, 0, ndt), None, 0.5)
        rec.add(label, rc.S_AT, "block mh_propose", rc.rel_max(P.cpu().numpy(), want) / se.ENSEMBLE_BAR[dtype], True, label)
        assert guards_intact(P_flat, P) and same_bytes(X.cpu().numpy(), Xh)
        if dtype == "float64":
            eng.forward_set_lineal(Al, bl)
            G = eng.forward_apply(X).cpu().numpy()
            rec.add(label, rc.S_AT, "block forward_apply", rc.rel_max(G, Al @ Xh + bl[:, None]) / cr.BAND, True, label)
        state["ran"] = True

    def gone(e):
        """behind the launch of step 5, whose set_problem dropped the proposal"""
        with pytest.raises(eng_mod.CesxError) as ei:
            eng.mh_propose(S_MH_STEP + 1, X)
        assert ei.value.code == eng_mod.ESTATE, str(ei.value)
        state["gone"] = True

    log = rc.run_sequence(eng_mod, eng, A, U0, probs, rc.S_STEPS, "cycle", rec, label, forms=forms, between={rc.S_AT: block},
                          before_result={rc.S_AT: gone})
    LOGS["S"].append((label, log))
    assert state == {"ran": True, "gone": True}
    with pytest.raises(eng_mod.CesxError) as ei:
        eng.mh_propose(S_MH_STEP + 2, X)
    assert ei.value.code == eng_mod.ESTATE
    eng.close()


# ---- T ------------------------------------------------------------------------------------------------------------------------

T_K = 3                          # GPs of the emulator image, columns of B (tests/test_gpu_engine_state.py)
T_JT = 17
T_ORDER = [b for b in rc.T_BLOCKS if b != "all"]


class TStages:
    """The inputs of T's blocks at one shape -- a block's own, fixed for the sequence, none of them the Calibrate state -- and the
    blocks.  ``run`` enqueues one block on an engine and returns its outputs as they are (device tensors are read when the
    sequence has ended, so that a block that does not synchronise by itself leaves the step in flight alone)."""

    def __init__(self, shape, prob, blocks):
        from ces_amd import emulate as em
        self.shape, self.prob, self.blocks = shape, prob, blocks
        p, n, J, dtype = shape
        ndt = np.dtype(dtype)
        rng = np.random.default_rng([rc.SEED, p, n, J, 11])
        self.X = (prob["mu"] + 0.5 * rng.standard_normal((p, J))).astype(ndt)
        self.A = (rng.standard_normal((n, p)) / np.sqrt(p)).astype(ndt)
        self.b = rng.standard_normal(n).astype(ndt)
        self.S = 0.3 * np.linalg.cholesky(prob["sigma"]) / np.sqrt(p)
        self.Ud = rng.standard_normal((p, J)).astype(ndt)
        enka = gc.random_gps(rng, p, T_K, T_JT, "Matern32")
        self.img = em.device_image(enka, enka.gpmodels)
        self.B = np.ascontiguousarray(np.linalg.qr(rng.standard_normal((n, T_K)))[0] * np.exp(rng.uniform(-2.0, 1.0, T_K)))
        self.g0 = prob["y"] + 0.1 * rng.standard_normal(n)
        self.proj = em.project_sigma(prob["Gamma"], self.B, self.g0, prob["y"])
        self.Xf, self.Yf = gc.fit_problem(rng, T_JT, p, 2)
        self.theta = np.hstack([np.full((2, 1), 1.3), np.tile(1.0 + 0.25 * (np.arange(p) % 8), (2, 1)), np.full((2, 1), 1e-3)])
        if "gp_run" in blocks:
            enka_n = gc.random_gps(rng, p, n, T_JT, "Matern32")
            self.img_n = em.device_image(enka_n, enka_n.gpmodels)
        if "l96" in blocks:
            params, starts = lc.class_params("lorenz96", (5, 3))
            self.Ul, self.W0 = np.array(params[:, :J]).astype(ndt), np.array(starts[:, :J], dtype=np.float64)
            self.t = lc.times(0.2, n=21)

    def models(self):
        """the host models of one engine (a model object keeps the token of the engine it was installed in)"""
        m = types.SimpleNamespace()
        if "darcy" in self.blocks:
            p, n = self.shape[:2]
            m.darcy, m.darcy_s = dc.make_model(4, p, n), dsc.make_model(4, p, n, "streamed")
        if "l96" in self.blocks:
            m.l96 = lc.make_model("lorenz96_hom", T=0.2)
            m.l96.n_slow, m.l96.n_fast = 5, 3
            m.l96.n_state = 5 * (3 + 1)
        return m

    def dev(self, eng, a):
        import torch
        return torch.as_tensor(np.ascontiguousarray(a), device=eng.device)

    def run(self, eng, m, name, call, W_in):
        """Block ``name`` on ``eng`` as call number ``call`` of the sequence (its MH step indices); W_in: the carried Lorenz
        state.  Returns {key: device tensor or host value}."""
        out = {}
        for sub in (T_ORDER if name == "all" else [name]):
            if sub in self.blocks:
                out.update(getattr(self, "_" + sub)(eng, m, rc.T_MH_STEP0 + 16 * call, W_in))
        return out

    def _lineal(self, eng, m, base, W):
        eng.forward_set_lineal(self.A, self.b)
        return dict(fwd=eng.forward_apply(self.dev(eng, self.X)))

    def _darcy(self, eng, m, base, W):
        return dict(darcy=m.darcy.forward_device(eng, self.dev(eng, self.Ud)))

    def _darcy_streamed(self, eng, m, base, W):
        m.darcy.invalidate_device()
        m.darcy.ensure_installed(eng)                   # the resident map first: the streamed install replaces it
        m.darcy_s.invalidate_device()
        out = m.darcy_s.forward_device(eng, self.dev(eng, self.Ud))
        assert eng.darcy_workspace_bytes() > 0
        return dict(darcy_streamed=out)

    def _l96(self, eng, m, base, W):
        m.l96.ensure_installed(eng, self.t)
        G, W_out, info = eng.l96_apply(self.dev(eng, self.Ul), W if not isinstance(W, np.ndarray) else self.dev(eng, W))
        return dict(l96_G=G, l96_W=W_out, l96_info=info)

    def _gp(self, eng, m, base, W):
        eng.gp_set(self.img)
        mean, var = eng.gp_predict(self.dev(eng, self.X))
        return dict(gp_mean=mean, gp_var=var)

    def _chain_out(self, eng, tag, U, **more):
        steps, rate, per = eng.mh_stats(per_chain=True)
        out = {tag + "_U": U, tag + "_phi": eng.mh_phi(), tag + "_steps": np.array([steps]), tag + "_rate": np.array([rate]),
               tag + "_count": per}
        out.update({tag + "_" + k: v for k, v in more.items()})
        return out

    def _mh(self, eng, m, base, W):
        eng.forward_set_lineal(self.A, self.b)
        eng.mh_set_proposal(None, self.S)
        U = self.dev(eng, self.X).clone()
        eng.mh_start(U, eng.forward_apply(U))
        for k in range(2):
            P = eng.mh_propose(base + k, U)
            eng.mh_accept(base + k, U, P, eng.forward_apply(P))
        return self._chain_out(eng, "mh", U, P=P)

    def _gp_mode(self, eng, mode, base):
        eng.mh_set_proposal(None, self.S)
        eng.gp_set(self.img)
        U = self.dev(eng, self.X).clone()
        mean, var = eng.gp_predict(U)
        eng.gp_start(mode, U, mean, var)
        for k in range(2):
            P = eng.mh_propose(base + k, U)
            mp, vp = eng.gp_predict(P)
            eng.gp_accept(mode, base + k, U, P, mp, vp)
        return self._chain_out(eng, "gp_" + mode, U, P=P, mean=mp, var=vp)

    def _gp_dense(self, eng, m, base, W):
        eng.gp_dense_set(self.B, self.g0, True)
        return self._gp_mode(eng, "dense", base + 2)

    def _gp_proj(self, eng, m, base, W):
        eng.gp_proj_set(*self.proj, True)
        return self._gp_mode(eng, "proj", base + 4)

    def _gp_run(self, eng, m, base, W):
        import torch
        eng.mh_set_proposal(None, self.S)
        eng.gp_set(self.img_n)
        U = self.dev(eng, self.X).clone()
        mean, _ = eng.gp_predict(U, var=False)
        eng.gp_start("gamma", U, mean)
        trace = torch.empty((5, self.shape[0], self.shape[2]), dtype=eng.torch_dtype, device=eng.device)
        eng.gp_run("gamma", base + 6, 5, U, trace=trace)
        return self._chain_out(eng, "gp_run", U, trace=trace)

    def _gpfit(self, eng, m, base, W):
        nt = eng.gpfit_set(self.Xf, self.Yf, 2, True, "zero")
        assert self.theta.shape == (2, nt)
        lml, grad, status = eng.gpfit_eval([1, 0], self.theta)
        assert np.all(status == 0), status
        return dict(fit_lml=lml, fit_grad=grad, fit_status=status)


def host(v):
    return v if isinstance(v, np.ndarray) else v.cpu().numpy()


@pytest.mark.parametrize("fam", cr.FAMILIES)
@pytest.mark.parametrize("run", rc.T_RUNS, ids=[r[0].replace(" ", "-") for r in rc.T_RUNS])
def test_sequence_t(eng_mod, run, fam):
    name, shape, blocks, dense = run
    A, U0, probs = rc.t_problem(fam, shape, dense)
    prob = probs[0]
    forms = forms_of(name.split()[0], rc.T_STEPS, probs)
    st = TStages(shape, prob, blocks)
    between, before = rc.t_plan(blocks)
    eng = make_engine(eng_mod, shape)
    shared = st.models()
    calls, carried, rates = [], {"W": getattr(st, "W0", None)}, {}

    def hook(call, block):
        def f(e):
            assert e is eng
            out = st.run(eng, shared, block, call, carried["W"])
            calls.append((call, block, carried["W"], out))
            carried["W"] = out.get("l96_W", carried["W"])
        return f
    rec, label = RECS["T"], "T %s %s" % (name, fam)
    log = rc.run_sequence(eng_mod, eng, A, U0, probs, rc.T_STEPS, "cycle", rec, label, forms=forms,
                          between={i: hook(*v) for i, v in between.items()}, before_result={i: hook(*v) for i, v in before.items()})
    LOGS["T"].append((label, log))
    assert [c[0] for c in calls] == list(range(22))
    # every block call against the same calls on an engine that has had set_problem and nothing else
    for call, block, W_in, out in calls:
        fresh = make_engine(eng_mod, shape)
        fresh.set_problem(prob["y"], prob["Gamma"], prob["mu"], prob["sigma"], prob["ustar"])
        want = st.run(fresh, st.models(), block, call, W_in)
        assert sorted(want) == sorted(out) and out, (label, block)
        for key in sorted(out):
            a, b = host(out[key]), host(want[key])
            assert np.all(np.isfinite(b.astype(np.float64))), (label, block, key, "the fresh engine's output is not finite")
            rec.add(label, call // 2 + call % 2, "block %s %s" % (block, key), 0.0 if same_bytes(a, b) else np.inf, True,
                    (label, "call %d of the sequence" % call, block, key,
                     "differing entries: %d of %d" % (int(np.sum(a != b)) if a.shape == b.shape else -1, a.size)))
        if "l96_info" in out:
            assert np.all(host(out["l96_info"])[0] == 0)
        rates.update({(call, key): float(host(val)[0]) for key, val in out.items() if key.endswith("_rate")})
        fresh.close()
    eng.close()
    print("%s: accept rates of the chain blocks %.3f .. %.3f over %d block calls" % (label, min(rates.values()), max(rates.values()), len(rates)))
    assert any(0.0 < r < 1.0 for r in rates.values()), (label, "no chain block moved some chains and kept others", rates)


# ---- the drop-in object ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fam", cr.FAMILIES)
@pytest.mark.parametrize("name", sorted(rc.ENGINES))
def test_the_drop_in_object_through_the_rules_of_r(eng_mod, name, fam):
    """One ``sampling`` object (its engine from ``_get_engine``, created once) through R's rule list by eks_update /
    eks_update_aldi / eks_update_aldi_constant, against ONE OracleState carried across the same steps: its pseudo-time trace
    and first-step flag are the carried ones, not the table's.  The inputs of a step are its own (the array the object
    returned, read exactly).  E1's ensemble is smaller than 4 p: the object runs it on an fp64 engine, and is held to fp64's
    TOL there."""
    from ces_amd.calibrate import sampling
    p, n, J, dtype = rc.ENGINES[name]
    A, U0, probs = rc.problems(fam, p, n, J, dtype)
    prob = probs[0]
    eks = sampling(p, n, J)
    eks.engine_dtype, eks.seed = dtype, rc.SEED
    eks.mu, eks.sigma, eks.ustar = prob["mu"], prob["sigma"], prob["ustar"]
    eng = eks._get_engine()
    ndt = eng.np_dtype
    assert ndt.name == ("float64" if J < 4 * p else dtype)
    tol = rc.TOL[ndt.name]
    st = oc.OracleState(p, n, J, prob["mu"], prob["sigma"], prob["ustar"])
    update = {"aldi": eks.eks_update_aldi, "eks": eks.eks_update, "aldi_constant": eks.eks_update_aldi_constant}
    rng = np.random.default_rng([rc.SEED, p, n, J, 3])
    rec, label = RECS["drop-in"], "drop-in %s %s" % (name, fam)
    U, log = U0.astype(ndt).astype(np.float64), []
    for i, s in enumerate(rc.R_STEPS):
        if s["edit"]:
            U *= 1.03125                                   # in place, in the array the object returned: a fresh centring pass is due
        Uh = U.copy()
        Gh = rc.forward(A, Uh, ndt)
        xi = rng.standard_normal((p, J)).astype(ndt).astype(np.float64)
        kw = {k: v for k, v in s["kw"].items() if k == "time_step" or v is not None}
        st.trace_len = 1 if i == 0 else 2
        t_before = st.metrics["t"][-1] if i else None
        ref = oc.factored_step(st, prob["y"], Uh, Gh, prob["Gamma"], xi, update=s["update"], **kw)
        if kw["time_step"] == "mix":                       # the carried trace must not sit on a threshold of the rule
            assert abs(t_before - kw.get("spinup", 4.0)) > 1e-2 and abs(st.metrics["t"][-1] - 1.0) > 1e-2, (t_before, st.metrics["t"][-1])
        out = update[s["update"]](prob["y"], U, Gh, prob["Gamma"], i, xi=xi, **kw)
        assert eks._get_engine() is eng and out is not U and np.array_equal(U, Uh)
        rec.add(label, i, "whole U_next", rc.rel_max(out, ref) / tol, True, (label, s["update"], s["rule"]))
        rec.add(label, i, "whole t", abs(eks.metrics["t"][-1] - st.metrics["t"][-1]) / abs(st.metrics["t"][-1]) / tol, True,
                (label, eks.metrics["t"][-1], st.metrics["t"][-1]))
        log.append((-1 if s["update"] == "aldi_constant" else eng.update_form(), eng.warm_inverse()))
        U = out
    assert len(eks.metrics["t"]) == len(st.metrics["t"]) == len(rc.R_STEPS)
    LOGS["drop-in"].append((label, log))
