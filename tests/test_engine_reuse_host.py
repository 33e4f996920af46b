"""The sequences of tests/reuse_cases.py without a device: the tables cover what they must, the stepper and its bars pass a
numpy stand-in for ``Engine`` that computes every stage in the engine dtype (with room: on fp32 the K2-from-inputs errors stay
under a tenth of their bar), and a stand-in that keeps ONE piece of state from the step before -- the stale values a reused
engine could serve -- leaves at least 4x a bar at the first step it does so, in at least one problem family."""
import ctypes
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import reuse_cases as rc  # noqa: E402
import test_dense_plans_host as dp  # noqa: E402
import test_gpu_calibrate_edges as ge  # noqa: E402

from oracle import calibrate_ref as cr  # noqa: E402
from oracle import philox  # noqa: E402

UPD_NAME = {0: "eks", 1: "aldi", 2: "aldi_constant"}
TS_NAME = {0: None, 1: "spectral", 2: "constant", 4: "mix"}
MUTANTS = ("stale_K", "stale_M", "stale_L", "stale_image_rows", "stale_whitening", "stale_y", "stale_Gw", "stale_ns_inverse",
           "stale_data_metrics")


def step_params(update="aldi", time_step=None, first_step=True, t_len=0, t_last=0.0, delta_t=None, spinup=4.0, switch=1.0,
                step_index=0, T=30):
    """ces_amd.engine.step_params without the library (the same fields, by name)"""
    return types.SimpleNamespace(update={v: k for k, v in UPD_NAME.items()}[update], time_step={v: k for k, v in TS_NAME.items()}[time_step],
                                 first_step=int(bool(first_step)), t_len=int(t_len), t_last=float(t_last),
                                 delta_t=float(delta_t if delta_t is not None else 1.0 / (T / 2)), spinup=float(spinup),
                                 switch_mult=float(switch), step_index=int(step_index))


MOD = types.SimpleNamespace(step_params=step_params)


class Done(Exception):
    """raised by a mutant stand-in in front of the step after the first one it served a stale value at"""


class NumpyEngine:
    """What the entry points of ces_amd.engine.Engine compute, by numpy: the Gram sums, the whitening product, the update and the
    per-particle metric sums in the ENGINE dtype (cr.moments_in_dtype, cr.update_in_dtype), K2 in fp64 (cr.dense_ref).
    ``stale``: one of MUTANTS -- that piece of state is served from the step (or problem) before wherever there is one;
    ``mutated`` lists the steps at which that happened."""

    def __init__(self, p, n_obs, J, dtype, seed=rc.SEED, stale=None):
        self.p, self.n_obs, self.J, self.seed, self.stale = p, n_obs, J, seed, stale
        self.np_dtype = np.dtype(dtype)
        self.torch_dtype = torch.float32 if self.np_dtype == np.float32 else torch.float64
        self.device = torch.device("cpu")
        self.prob = self.old_prob = self.shift = self.last = self.res = None
        self.chain = self.flipped = False
        self.form, self.steps_done, self.mutated = 0, 0, []

    # -- buffers and the problem
    def empty(self, rows):
        return torch.empty((rows, self.J), dtype=self.torch_dtype)

    def to_device(self, a, rows=None, tag=None):
        return a

    def set_problem(self, y, Gamma, mu, sigma, ustar):
        if self.mutated and self.steps_done > self.mutated[0]:
            raise Done
        new = dict(y=np.array(y, dtype=np.float64).ravel(), Gamma=np.array(Gamma, dtype=np.float64), mu=np.array(mu, dtype=np.float64).reshape(-1, 1),
                   sigma=np.array(sigma, dtype=np.float64), ustar=np.array(ustar, dtype=np.float64).reshape(-1, 1))
        if self.prob is not None and all(np.array_equal(new[k], self.prob[k]) for k in new):
            return
        self.old_prob, self.prob, self.shift = self.prob, new, None
        chain = ge.pick(self.p, self.n_obs, self.J, self.np_dtype.name, "aldi", None, dense_sigma=not cr.is_diagonal(new["sigma"]))[0] == 2
        self.flipped, self.chain = chain != self.chain and self.old_prob is not None, chain

    def _whitening(self, stale_ok=True):
        Lg, Li = cr.whitening(self.prob["Gamma"])
        if Lg is not None and stale_ok and self.stale == "stale_whitening" and self.old_prob is not None:
            Lo, Lio = cr.whitening(self.old_prob["Gamma"])
            if Lo is not None and not np.array_equal(Lo, Lg):
                self._mark()
                return Lo, Lio
        return Lg, Li

    def _mark(self):
        if self.steps_done not in self.mutated:
            self.mutated.append(self.steps_done)

    # -- K1
    def colsum(self, U, G):
        return torch.as_tensor(np.concatenate([[float(self.J)], U.numpy().astype(np.float64).sum(axis=1), G.numpy().astype(np.float64).sum(axis=1)]))

    def set_shift(self, sums):
        s = sums.numpy().copy()
        Lg, Li = self._whitening(stale_ok=False)
        if Lg is not None:
            s[1 + self.p:] = Li @ s[1 + self.p:]
        self.shift = cr.round_shift(s, self.np_dtype)

    def moments_len(self):
        return cr.moments_layout(self.p, self.n_obs)["len"]

    def moments_uu_len(self):
        return cr.moments_layout(self.p, self.n_obs)["uu_len"]

    def moments(self, U, G, out=None):
        assert self.shift is not None, "no centring shift"
        dt, p = self.np_dtype, self.p
        Uh, Gh = U.numpy().astype(np.float64), G.numpy().astype(np.float64)
        Lg, Li = self._whitening()
        Gw = Gh
        if Lg is not None:
            Gw = (Li.astype(dt) @ Gh.astype(dt)).astype(np.float64)
            if self.stale == "stale_Gw" and self.last is not None and self.last.get("Gw") is not None:
                Gw = self.last["Gw"]                 # the cache answers for the same pointer: the rows of the step before
                self._mark()
        self._Gw = Gw if Lg is not None else None
        self._rows = Gw
        mom = cr.moments_in_dtype(Uh, Gw, self.shift[:p], self.shift[p:], dt, 32 if dt == np.float32 else 16)
        buf = torch.zeros(self.moments_len(), dtype=torch.float64) if out is None else out
        buf[:len(mom)] = torch.as_tensor(mom)
        return buf

    def moments_uu_chol(self, prm, U, G, out=None):
        return torch.zeros(self.moments_len(), dtype=torch.float64) if out is None else out

    def moments_rest(self, U, G, mom):
        return self.moments(U, G, out=mom)

    def prefetch_noise(self, step_index):
        pass

    def draw_noise(self, step_index):
        return torch.as_tensor(philox.noise_block(self.p, self.J, self.seed, step_index, dtype=self.np_dtype).astype(self.np_dtype))

    # -- K2 + K3
    def _dense(self, prm, mom):
        upd = UPD_NAME[prm.update]
        prob = self.prob
        if self.stale == "stale_y" and self.old_prob is not None and not np.array_equal(self.old_prob["y"], prob["y"]):
            prob = dict(prob, y=self.old_prob["y"])
            self._mark()
        ts = {} if upd == "aldi_constant" else dict(time_step=TS_NAME[prm.time_step], delta_t=prm.delta_t, spinup=prm.spinup,
                                                    first_step=bool(prm.first_step), t_len=prm.t_len, t_last=prm.t_last)
        k2 = cr.dense_ref(mom.numpy(), self.shift, prob, upd, **ts)
        dd = {k: np.array(k2[k]) for k in ("ubar", "gbar", "C", "L", "K", "M")}
        for key in ("K", "M", "L"):
            if self.stale == "stale_" + key and self.last is not None:
                dd[key] = self.last["dd"][key]
                self._mark()
        return upd, prob, k2, dd

    def _metrics(self, dd, prob):
        dt, n = self.np_dtype, self.n_obs
        Lg, Li = cr.whitening(self.prob["Gamma"])
        if Lg is None:
            w, y, gbar = 1.0 / np.diag(prob["Gamma"]), prob["y"], dd["gbar"]
        else:
            w, y, gbar = np.ones(n), Li @ prob["y"], Li @ dd["gbar"]
        R = self._rows.astype(dt)
        out = []
        for c in (y, gbar):
            q = (w.astype(dt)[:, None] * (R - c.astype(dt)[:, None]) ** 2).sum(axis=0, dtype=dt).astype(np.float64)
            out.append(float((q * q).sum() / self.J))
        if self.stale == "stale_data_metrics" and self.last is not None:
            self._mark()
            return self.last["metrics"], out
        return out, out

    def _noise(self, prm, xi):
        return xi.numpy().astype(np.float64) if xi is not None else self.draw_noise(prm.step_index).numpy().astype(np.float64)

    def _publish(self, prm, k2, dd, hk, met, keep, out, res_h):
        t_new = hk if prm.first_step else hk + prm.t_last
        self.res = types.SimpleNamespace(hk=hk, t_new=t_new, bias=k2["bias"], self_bias=k2["self_bias"], radspec=k2["radspec"] or 0.0,
                                         bias_data=met[0], self_bias_data=met[1], status=0)
        out.copy_(torch.as_tensor(res_h.astype(self.np_dtype)))
        # the shift K2 predicts for the next step: the mean of what it is about to write (U), the data mean as it stands (G)
        pred = np.concatenate([[1.0], res_h.astype(np.float64).mean(axis=1), self.shift[self.p:]])
        self.shift = cr.round_shift(pred, self.np_dtype)
        self.last = dict(dd=dd, Gw=self._Gw, metrics=keep, P=self._extra.get("P"))
        self.steps_done += 1

    def apply(self, prm, mom, U, G, xi=None, out=None):
        upd, prob, k2, dd = self._dense(prm, mom)
        dt, J = self.np_dtype, self.J
        Uh, Gh, xi_h = U.numpy().astype(np.float64), G.numpy().astype(np.float64), self._noise(prm, xi)
        hk = k2["hk"]
        self.form = ge.pick(self.p, self.n_obs, J, dt.name, upd, TS_NAME[prm.time_step], dense_sigma=not cr.is_diagonal(prob["sigma"]))[0]
        kform = "eks" if upd == "eks" else cr.FORM_OF_UPDATE_FORM[self.form]
        P = cr._parts(kform, dd, hk, prob, J)
        self._extra = {}
        if kform == "eks":
            if self.stale == "stale_ns_inverse" and self.last is not None and self.last.get("P") is not None:
                P["P"] = self.last["P"]               # the inverse of the step before, accepted without its residual test
                P["PK"] = P["P"] @ P["K"]
                self._mark()
            self._extra = dict(P=P["P"])
        if self.stale == "stale_image_rows" and self.flipped and self.last is not None and "L" in cr.FORM_BLOCKS[kform]:
            # a change of layout without the zeroed image: rows of the other layout where this one writes nothing; the last
            # k-tile of the L block stands in for them (the factor of the step before)
            P["L"] = P["L"].copy()
            k0 = 16 * ((self.p - 1) // 16)
            P["L"][:, k0:] += np.tril(self.last["dd"]["L"])[:, k0:]
            self.flipped = False
            self._mark()
        res_h = np.asarray(cr._eval(kform, P, Uh, Gh, xi_h, None, dt=dt), dtype=np.float64)
        met, keep = self._metrics(dd, prob)
        self._dd = dd
        if self._extra.get("P") is None and self.last is not None and self.last.get("P") is not None:
            self._extra = dict(P=self.last["P"])      # (an EKS inverse outlives the steps of other rules)
        self._publish(prm, k2, dd, hk, met, keep, out, res_h)
        return out

    def apply_drift(self, prm, mom, U, G, out):
        upd, prob, k2, dd = self._dense(prm, mom)
        drift = cr.update_in_dtype("drift", dd, None, U.numpy().astype(np.float64), G.numpy().astype(np.float64), None, prob,
                                   self.np_dtype, J=self.J, switch=prm.switch_mult).astype(self.np_dtype)
        out.copy_(torch.as_tensor(drift))
        self._pending = (prob, k2, dd) + self._metrics(dd, prob)
        self._dd = dd
        return torch.tensor([float(np.max(np.abs(drift.astype(np.float64))))], dtype=torch.float64)

    def apply_finish(self, prm, absmax, U, xi, out):
        prob, k2, dd, met, keep = self._pending
        hk = 0.1 / float(absmax[0])
        res_h = cr.update_in_dtype("finish", dd, hk, U.numpy().astype(np.float64), None, self._noise(prm, xi), prob, self.np_dtype,
                                   J=self.J, drift=out.numpy().astype(np.float64))
        self._extra = dict(P=self.last["P"]) if self.last is not None and self.last.get("P") is not None else {}
        self._publish(prm, k2, dd, hk, met, keep, out, np.asarray(res_h, dtype=np.float64))
        return out

    def step(self, prm, U, G, xi=None, out=None, recenter=True):
        if recenter:
            self.set_shift(self.colsum(U, G))
        return self.apply(prm, self.moments(U, G), U, G, xi, out=out)

    def result(self):
        return self.res

    def debug_dense(self):
        return {k: v.copy() for k, v in self._dd.items()}

    def update_form(self):
        return self.form

    def warm_inverse(self):
        return 0


def forms_of(name, steps, probs):
    return [rc.expected_form(name, s, probs[s["prob"]]) for s in steps]


# ---- the tables ---------------------------------------------------------------------------------------------------------------

def test_the_sequence_tables_cover_what_they_must():
    R = [(s["update"], s["rule"]) for s in rc.R_STEPS]
    assert R == [("aldi", "default"), ("aldi", "default"), ("aldi", "constant_dt"), ("aldi", "spectral"), ("aldi", "default"),
                 ("eks", "default"), ("eks", "constant_dt"), ("aldi", "default"), ("aldi_constant", "default"),
                 ("aldi", "mix_late_recompute"), ("aldi", "default"), ("eks", "default")]
    assert rc.R_STEPS[0]["first"] and rc.R_STEPS[0]["recenter"] and not rc.R_STEPS[1]["recenter"]
    assert sum(s["edit"] and s["recenter"] for s in rc.R_STEPS) == 1 and 0 < [s["edit"] for s in rc.R_STEPS].index(True) < 11
    assert {rc.noise_of(i) for i in range(12)} == set(rc.NOISE)
    # the cycling flow pairs every flow with more than one noise mode
    pairs = {(rc.flow_of("cycle", i), rc.noise_of(i)) for i in range(12)}
    assert all(len({nz for f, nz in pairs if f == fl}) >= 2 for fl in rc.FLOWS), pairs
    assert {rc.flow_of("cycle", i) for i in range(12)} == set(rc.FLOWS)
    forms = {}
    for name, (p, n, J, dtype) in rc.ENGINES.items():
        _, _, probs = rc.problems("data", p, n, J, dtype)
        forms[name] = forms_of(name, rc.R_STEPS, probs)
    assert set(forms["E1"]) == {2, 0, -1} and set(forms["E2"]) == {1, 0, -1} and set(forms["E3"]) == {0, -1}
    assert forms["E1"][:5] == [2, 2, 0, 0, 2] and forms["E2"][:5] == [1, 1, 0, 0, 1]
    assert ge.pick(96, 80, 1028, "float32") == (1, "update2") and 1028 % 32 != 0
    # P: chain flips off (a dense Sigma) and on again on E1; whitening comes, changes and goes
    p, n, J, dtype = rc.ENGINES["E1"]
    _, _, probs = rc.problems("prior", p, n, J, dtype, "P")
    fp = forms_of("E1", rc.P_STEPS, probs)
    assert fp == [2, 2, 1, 1, 2, 2, 0, 2, 2, 2, 2, 2, 2]
    chain = [f == 2 for f, s in zip(fp, rc.P_STEPS) if s["update"] == "aldi"][::2]
    assert sum(a != b for a, b in zip(chain, chain[1:])) == 2
    dense_g = [not cr.is_diagonal(q["Gamma"]) for q in probs]
    assert dense_g == [False, False, True, True, True, False] and not np.array_equal(probs[2]["Gamma"], probs[3]["Gamma"])
    assert all(np.array_equal(probs[3][k], probs[4][k]) for k in ("Gamma", "sigma")) and not np.array_equal(probs[3]["y"], probs[4]["y"])
    assert all(s["recenter"] for i, s in enumerate(rc.P_STEPS) if i == 0 or s["prob"] != rc.P_STEPS[i - 1]["prob"])
    assert rc.S_STEPS[rc.S_AT]["recenter"] and rc.S_STEPS[rc.S_AT]["update"] == "eks"


def test_the_rules_of_sequence_r_reach_every_route_of_the_dense_plan():
    """What this shows and what it does not: the facts handed to cesx_debug_dense_plan are written here, per rule of R, for E1 in
    the steady state the benchmark fixture of tests/test_dense_plans_host.py names (chol(C) in flight for a step and for the
    drift, L into the image for aldi, d_L left out behind a tail step) -- they are NOT read from an engine along R.  For such
    facts the planner gives the Tail, General, Finish and NoiseOnly routes, the spectral block and both hk-dependent inverses: R's
    rule list can reach every route; which route a given step of a given flow took on a device is not observable through the
    ABI and is not asserted anywhere."""
    from ces_amd import build, engine
    build.build_lib()
    lib = engine.load_library()
    facts, out = (ctypes.c_int32 * dp.NF)(), (ctypes.c_int32 * dp.NP)()
    seen = []
    for s in rc.R_STEPS:
        upd = {v: k for k, v in UPD_NAME.items()}[s["update"]]
        ts = {v: k for k, v in TS_NAME.items()}[s["kw"]["time_step"]]
        for ph in ((1, 2) if upd == 2 else (0,)):
            f = dp.base()
            f[dp.UPDATE], f[dp.PHASE], f[dp.TIME_STEP], f[dp.UPD_OK] = upd, ph, ts, 1
            f[dp.INFLIGHT] = int(ph != 2)
            f[dp.IMG] = int(upd == 1)
            f[dp.IMAGE_ONLY] = int(f[dp.IMG] and ts == 0)
            facts[:] = f
            assert lib.cesx_debug_dense_plan(facts, out) == 0
            seen.append(list(out))
    assert {dp.ROUTE[q[0]] for q in seen} == set(dp.ROUTE), {dp.ROUTE[q[0]] for q in seen}
    assert any(q[8] for q in seen) and any(q[9] for q in seen) and any(q[10] for q in seen)


# ---- the dry run --------------------------------------------------------------------------------------------------------------

def dry(name, which, fam, flow, between=None):
    p, n, J, dtype = rc.ENGINES[name]
    A, U0, probs = rc.problems(fam, p, n, J, dtype, which)
    steps = {"R": rc.R_STEPS, "P": rc.P_STEPS, "S": rc.S_STEPS}[which]
    rec = rc.Record()
    rc.run_sequence(MOD, NumpyEngine(p, n, J, dtype), A, U0, probs, steps, flow, rec, "%s %s %s %s" % (which, name, fam, flow),
                    forms=forms_of(name, steps, probs), between=between)
    room(rec, dtype)


@pytest.mark.parametrize("fam", cr.FAMILIES)
@pytest.mark.parametrize("flow", rc.FLOWS + ("cycle",))
@pytest.mark.parametrize("name", sorted(rc.ENGINES))
def test_dry_run_of_sequence_r(name, flow, fam):
    dry(name, "R", fam, flow)


@pytest.mark.parametrize("fam", cr.FAMILIES)
@pytest.mark.parametrize("name", ["E1", "E3"])
def test_dry_run_of_sequence_p(name, fam):
    dry(name, "P", fam, "cycle")


@pytest.mark.parametrize("fam", cr.FAMILIES)
@pytest.mark.parametrize("name", ["E1", "E3"])
def test_dry_run_of_sequence_s(name, fam):
    """S's Calibrate steps.  The stand-in has no Sample stage; what the block leaves behind for the Calibrate steps is there: it
    sets a problem of its own on the engine (``mh_case`` does), so step 5 meets a problem set again and no centring shift."""
    p, n, J, dtype = rc.ENGINES[name]
    other = rc.problems(fam, p, n, J, dtype, "P")[2][4]
    dry(name, "S", fam, "cycle", between={rc.S_AT: lambda e: e.set_problem(other["y"], other["Gamma"], other["mu"], other["sigma"], other["ustar"])})


@pytest.mark.parametrize("fam", cr.FAMILIES)
@pytest.mark.parametrize("run", rc.T_RUNS, ids=[r[0].replace(" ", "-") for r in rc.T_RUNS])
def test_dry_run_of_sequence_t(run, fam):
    """T's Calibrate steps with the reference alone: no-op blocks, still called through both hooks, in the table's order (every
    block in ``before_result`` of a step and then in ``between`` in front of the next); every check of every step passes."""
    name, shape, blocks, dense = run
    p, n, J, dtype = shape
    A, U0, probs = rc.t_problem(fam, shape, dense)
    assert (not cr.is_diagonal(probs[0]["Gamma"]), not cr.is_diagonal(probs[0]["sigma"])) == dense
    between, before = rc.t_plan(blocks)
    assert sorted(between) == list(range(1, 12)) and sorted(before) == list(range(11))
    assert all(before[i - 1][1] == between[i][1] == blocks[(i - 1) % len(blocks)] for i in range(1, 12))
    assert {b for _, b in between.values()} == set(blocks)
    eng, calls = NumpyEngine(p, n, J, dtype), []

    def hook(where, i, call, block):
        def f(e):
            assert e is eng
            calls.append((call, where, i, block, e.steps_done))
        return f
    rec = rc.Record()
    forms = forms_of(name.split()[0], rc.T_STEPS, probs)
    rc.run_sequence(MOD, eng, A, U0, probs, rc.T_STEPS, "cycle", rec, "T %s %s" % (name, fam), forms=forms,
                    between={i: hook("between", i, *v) for i, v in between.items()},
                    before_result={i: hook("before_result", i, *v) for i, v in before.items()})
    # 22 calls in the table's order; a ``before_result`` call of step i runs when the stand-in has finished i + 1 steps (the
    # launch of step i is behind it), the ``between`` call in front of step i when it has finished i
    assert [c[0] for c in calls] == list(range(22))
    assert all(done == (i + 1 if where == "before_result" else i) for _, where, i, _, done in calls), calls
    if name == "T":
        assert set(forms) == {0, -1}
    else:
        assert set(forms) == ({2, 0, -1} if not dense[1] else {1, 0, -1})
    room(rec, dtype)


def test_the_new_hook_leaves_present_callers_alone():
    """``before_result=None`` (the default) and an empty table record the same ratios as a call without the argument."""
    p, n, J, dtype = rc.ENGINES["E3"]
    A, U0, probs = rc.problems("data", p, n, J, dtype)
    rows = []
    for kw in ({}, dict(before_result=None), dict(before_result={})):
        rec = rc.Record()
        rc.run_sequence(MOD, NumpyEngine(p, n, J, dtype), A, U0, probs, rc.R_STEPS[:4], "cycle", rec, "R", **kw)
        rows.append(rec.rows)
    assert rows[0] == rows[1] == rows[2]


def room(rec, dtype):
    """on fp32 the K2-from-inputs errors stay under a tenth of their bar: the bar has room before a device is involved"""
    k2 = max(r for _, _, part, r in rec.rows if part.startswith("K2 ") and part != "K2 L")
    print("worst K2-from-inputs error / bar: %.3g; worst K3 / bound: %.3g" % (k2, max(r for _, _, part, r in rec.rows if part.startswith("K3 "))))
    if dtype == "float32":
        assert k2 < 0.1, k2


@pytest.mark.parametrize("name", ["E1", "E3"])
def test_dry_run_pipelined_equals_unpipelined(name):
    p, n, J, dtype = rc.ENGINES[name]
    A, U0, probs = rc.problems("data", p, n, J, dtype)
    rows = [rc.run_pipelined(MOD, NumpyEngine(p, n, J, dtype), A, U0, probs, rc.R_STEPS, rc.Record(), "pipe", pl) for pl in (False, True)]
    for (ua, ra), (ub, rb) in zip(*rows):
        assert np.array_equal(ua, ub) and np.array_equal(ra, rb)


# ---- stale state ---------------------------------------------------------------------------------------------------------------

MUTANT_RUNS = {"stale_K": "R", "stale_M": "R", "stale_L": "R", "stale_ns_inverse": "R", "stale_data_metrics": "R",
               "stale_image_rows": "P", "stale_whitening": "P", "stale_y": "P", "stale_Gw": "P"}


@pytest.mark.parametrize("stale", MUTANTS)
def test_stale_state_leaves_four_times_a_bar(stale):
    """Each mutant on E1 (the engine with every form), both families: at the FIRST step the stale value is served, some check
    is at 4x its bar or beyond in at least one family (the factor of calibrate_ref.mutants)."""
    seen = {}
    for fam in cr.FAMILIES:
        rec = rc.Record()
        p, n, J, dtype = rc.ENGINES["E1"]
        eng = NumpyEngine(p, n, J, dtype, stale=stale)
        label = "%s %s %s" % (MUTANT_RUNS[stale], fam, stale)
        A, U0, probs = rc.problems(fam, p, n, J, dtype, MUTANT_RUNS[stale])
        with pytest.raises(Done):
            rc.run_sequence(MOD, eng, A, U0, probs, rc.P_STEPS if MUTANT_RUNS[stale] == "P" else rc.R_STEPS, "cycle", rec, label, strict=False)
        assert eng.mutated, (stale, "the mutant never took effect")
        at = rec.at(label, eng.mutated[0])
        before = [r for lab, i, part, r in rec.rows if i < eng.mutated[0]]
        assert all(r <= 1.0 for r in before), (stale, "a check fails before the stale value is served")
        part = max(at, key=at.get)
        seen[fam] = (eng.mutated[0], part, at[part])
    print("MUTANT %-20s %s" % (stale, "   ".join("%s: step %d, %s at %.3g x its bar" % ((fam,) + v) for fam, v in seen.items())))
    assert max(v[2] for v in seen.values()) >= 4.0, (stale, seen)


# ---- the Sample block of sequence S: its seeds leave out no chain-step ------------------------------------------------------

class ReferenceMH:
    """The MH entry points ``mh_case`` of tests/test_gpu_sample_edges.py drives, answered by the fp64 reference alone
    (oracle/stage_ref.py): what the device is compared with, standing in for it."""

    def __init__(self, p, n_obs, J, dtype):
        self.p, self.n_obs, self.J, self.np_dtype = p, n_obs, J, np.dtype(dtype)
        self.torch_dtype = torch.float32 if self.np_dtype == np.float32 else torch.float64
        self.device = torch.device("cpu")

    def set_problem(self, y, Gamma, mu, sigma, ustar):
        self.y, self.gw, self.mu, self.sw = np.asarray(y, dtype=np.float64), 1.0 / np.diag(Gamma), np.asarray(mu, dtype=np.float64).ravel(), 1.0 / np.diag(sigma)

    def mh_set_proposal(self, kind, S, beta=0.5):
        self.kind = kind

    def _phi(self, X, G):
        from oracle import stage_ref as sr
        X, G = X.numpy().astype(np.float64), G.numpy().astype(np.float64)
        return sr.mh_phi(G, self.y, self.gw) if self.kind == "pCN" else sr.mh_phi(G, self.y, self.gw, X, self.mu, self.sw)

    def mh_start(self, U, G):
        self.phi, self.count, self.calls = self._phi(U, G), np.zeros(self.J, dtype=np.uint64), 0

    def mh_accept(self, step_index, U, P, GP, logu=None):
        phi_p = self._phi(P, GP)
        acc = logu.numpy() < self.phi - phi_p
        idx = torch.as_tensor(np.flatnonzero(acc))
        U[:, idx] = P[:, idx]
        self.phi = np.where(acc, phi_p, self.phi)
        self.count += acc.astype(np.uint64)
        self.calls += 1

    def mh_stats(self, per_chain=False):
        return self.calls, float(self.count.sum()) / (self.calls * self.J), self.count.copy()


@pytest.mark.parametrize("kind", [None, "pCN"], ids=["RW", "pCN"])
@pytest.mark.parametrize("name", ["E1", "E3"])
def test_the_sample_block_of_sequence_s_leaves_out_no_chain_step(name, kind):
    """Sequence S runs ``mh_case`` at the engines' own shapes between two Calibrate steps and wants no chain-step left out as a
    tie: at its seeds the reference alone has none (and some chains move, some do not: ``mh_case`` asserts that)."""
    import test_gpu_sample_edges as se
    p, n, J, dtype = rc.ENGINES[name]
    ref = se.mh_case(types.SimpleNamespace(Engine=lambda *a, **k: ReferenceMH(p, n, J, dtype)), dtype, p, n, J, kind, part="S host")
    assert ref.left_out == 0 and ref.chain_steps == se.STEPS * J
