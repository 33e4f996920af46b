"""One engine driven through a sequence of steps: the tables and the stepper, written for a device engine (``ces_amd.engine``) and
run by tests/test_engine_reuse_host.py against a numpy stand-in for the engine and by tests/test_gpu_engine_reuse.py against the
engine itself on a device (NOTEBOOK.md, "Tests: one engine across rules, problems and stages" and "Tests: the engine-reuse
sequences on a device").

Production keeps ONE engine for the life of a ``calibrate.sampling`` object, calls ``set_problem`` before every step and changes
route whenever the caller changes the rule or the time step.  What a step returns then depends on state that outlives a step in
``struct Engine`` (ces_amd/csrc/cesx_internal.h): the factorisation in flight and the layout of the coefficient image, the warm
started inverses, the whitening cache, the predicted centring shift, the deferred metric finalisation, the prefetched noise
blocks, the MH buffers that share the update kernels.  A stale value in any of them gives a finite, plausible U_next.

The stepper drives one engine through a list of steps.  The inputs of a step are its own: U is the tensor the previous step
returned, read back exactly; G = GAIN (A U + 0.05 sin(A U)) of that read-back U in fp64, rounded to the engine dtype; U, G and xi live
in the same three device tensors for the whole sequence (overwritten in place), the outputs alternate between two.  After each
step, against fp64 FROM THAT STEP'S OWN INPUTS (bounds: oracle/calibrate_ref.py):

1. K3     U_next against ``update_ref`` of the device's dense state, elementwise |err| <= (c_update eps [+ BAND]) B
2. K2     ubar, gbar, C, K, M, hk, t, bias, self_bias (radspec) of the device against ``dense_from_inputs``: relative to each
          array's maximum, BAND for an fp64 engine, the project's fp32 bar 1e-3 for an fp32 one (the moments carry fp32 Gram
          rounding; a stale array is off by a part in ten or a hundred); L against numpy's factor of the device's C at BAND
3. data   bias_data, self_bias_data against ``data_metrics_ref`` at ``c_metric``
4. whole  U_next against oracle/ces_numpy.py ``factored_step`` at TOL64 / TOL32
5. in place  U and G unchanged, the guards around all five buffers intact

Every comparison is recorded as its ratio to its bar (<= 1 passes); ``strict=False`` records without asserting (the mutants of
the host module)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from edge_helpers import guarded, guards_intact, put  # noqa: E402
import test_gpu_calibrate_edges as ge  # noqa: E402

from oracle import calibrate_ref as cr  # noqa: E402
from oracle import ces_numpy as oc  # noqa: E402
from oracle import philox  # noqa: E402

TOL = {"float64": 1e-6, "float32": 1e-3}          # TOL64 / TOL32 of tests/test_gpu_parity.py (BASELINE.json)
K2_BAR = {"float64": cr.BAND, "float32": 1e-3}
SEED = 77
STEP0 = 40                                        # Philox step index of a sequence's first step
ENGINES = {"E1": (256, 64, 512, "float32"),       # ALDI / default: the chained form 2
           "E2": (96, 80, 1028, "float32"),       # ragged J (no whole Gram tiles): form 1
           "E3": (33, 17, 1004, "float64")}       # form 0 throughout
FLOWS = ("step", "split", "sharded")
NOISE = ("injected", "engine", "ahead")
# The forward map of a sequence is G = GAIN (A U + 0.05 sin(A U)).  With GAIN = 1 (the map of ``cr.family``) the 'prior' family's
# default time step hk = 1 / ||D||_F is 4.9 on E1 while lambda_max(C Sigma^{-1}) = 0.74: hk lambda_max > 2, explicit ALDI is
# unstable and twelve steps take cond(C) to 2e8, out of the range fp32 moments resolve.  ||D||_F grows with the square of the gain,
# so GAIN = 4 brings hk to 0.2 (hk lambda_max = 0.15 .. 0.6 over the sequence; both families, all three engines: cond(C) <= 2e2).
GAIN = 4.0
T_PREV = [0.3]                                    # pseudo-time trace of a step that is not the first and whose rule names none


def step(update, rule="default", recenter=False, first=False, edit=False, prob=0):
    kw, t_prev = ge.TS_RULES[rule]
    return dict(update=update, rule=rule, kw=kw, t_prev=[] if first else (list(t_prev) or list(T_PREV)), recenter=recenter,
                first=first, edit=edit, prob=prob)


# R: the rules on one problem.  Step 11 meets an EKS inverse that is five steps old.
R_STEPS = [step("aldi", first=True, recenter=True), step("aldi"), step("aldi", "constant_dt"), step("aldi", "spectral"),
           step("aldi"), step("eks"), step("eks", "constant_dt"), step("aldi", recenter=True, edit=True), step("aldi_constant"),
           step("aldi", "mix_late_recompute"), step("aldi"), step("eks")]
# S: the same with another stage on the engine between steps 4 and 5 (the engine's problem is set again: a fresh shift)
S_AT = 5
S_STEPS = [dict(s, recenter=s["recenter"] or i == S_AT) for i, s in enumerate(R_STEPS)]
# P: six problems on one engine, two aldi / default steps each (the second on the predicted shift), an eks step behind P2
P_STEPS = []
for _k in range(6):
    P_STEPS += [step("aldi", first=not P_STEPS, recenter=True, prob=_k), step("aldi", prob=_k)]
    if _k == 2:
        P_STEPS.append(step("eks", prob=_k))
P_DENSE = [(False, False), (False, True), (True, False), (True, False), (True, False), (False, False)]      # (dense Gamma, dense Sigma)

# T: every other stage of the engine between Calibrate steps that leave the PROBLEM alone: the step behind a block runs on the
# predicted shift, on warm inverses, possibly with a noise block drawn ahead, and must not notice the block.  R's steps under flow
# 'cycle', one problem per shape with a dense Gamma (whitening live) and a dense Sigma (the dense prior live).  No block calls
# set_problem with other values; the stepper sets the same problem again before every step (a no-op in the engine), and a block
# sets its own proposal and descriptors whenever it runs.
T_STEPS = R_STEPS
T_ENGINE = (4, 5, 65, "float64")                  # the smallest shape every stage installs at (tests/test_gpu_engine_state.py)
# the blocks, in the order they are taken (cycling when they run out).  At step i >= 1 block (i - 1) % len runs in ``between``
# in front of step i AND in ``before_result`` of step i - 1 (behind the launch of step i - 1, before its result is read).
T_BLOCKS = ("lineal",          # forward_apply of the installed linear map
            "darcy",           # Darcy resident, K = 4: darcy_apply
            "darcy_streamed",  # Darcy streamed, K = 4: a re-install across solvers, then apply
            "l96",             # homogeneous Lorenz '96 at (5, 3): l96_apply with the carried W
            "gp",              # gp_set with J_t = 17, gp_predict with variance
            "mh",              # mh_set_proposal RW on the dense prior, mh_start, 2 x (mh_propose engine noise, mh_accept device
            #                    uniform), mh_phi, mh_stats
            "gp_dense",        # gp_dense_set, gp_start('dense'), 2 x gp_accept
            "gp_proj",         # gp_proj_set, gp_start('proj'), 2 x gp_accept
            "gp_run",          # fused chains: gp_run of 5 steps in mode 'gamma' (n_gp = n_obs; 256 (3 p + 32 + 2 n) + 8192 B of LDS)
            "gpfit",           # gpfit_set with J_t = 17, 2 GPs, gpfit_eval
            "all")             # all of the above, one after another
# E1 (256, 64, 512) fp32, after include/cesx.h: the Darcy maps need p <= K^2 (K = 4: p <= 16); the Lorenz '96 map needs n_obs = 5
# or 5 n_slow; cesx_gp_run in mode 'gamma' needs n_gp = n_obs = 64 GPs and 256 (3 * 256 + 32 + 2 * 64) + 8192 = 245 760 B of
# LDS > 160 KiB (CESX_EUNSUPPORTED).  The others carry no limit that E1 passes: k <= n_obs <= 128 (dense), k <= 128 (proj).
T_BLOCKS_E1 = ("lineal", "gp", "mh", "gp_dense", "gp_proj", "gpfit", "all")
# (name, engine shape, blocks, (dense Gamma, dense Sigma)).  E1 with a dense Sigma takes form 1 and never the chained form 2
# (``pick``: form 2 needs a diagonal Sigma), so E1 runs twice: with the diagonal Sigma (forms 2 and 0) and with the dense one.
T_RUNS = (("T", T_ENGINE, T_BLOCKS, (True, True)),
          ("E1 diagonal Sigma", ENGINES["E1"], T_BLOCKS_E1, (True, False)),
          ("E1 dense Sigma", ENGINES["E1"], T_BLOCKS_E1, (True, True)))
T_MH_STEP0 = 1000                                 # MH step index of the sequence's first block call; each call takes 16


def t_plan(blocks, n_steps=len(R_STEPS)):
    """(between, before_result): {step: (call number, block name)} of sequence T.  The call number counts the block calls of the
    sequence in the order they run; a call's MH step indices start at T_MH_STEP0 + 16 * call number."""
    between, before = {}, {}
    for i in range(1, n_steps):
        name = blocks[(i - 1) % len(blocks)]
        before[i - 1] = (2 * (i - 1), name)
        between[i] = (2 * (i - 1) + 1, name)
    return between, before


def t_problem(fam, shape, dense):
    """(A, U0, [problem]) of one run of T"""
    p, n, J, dtype = shape
    d = cr.family(fam, p, n, J, dtype, dense_gamma=dense[0], dense_sigma=dense[1])
    return d["A"], d["U0"], [{k: d[k] for k in ("y", "Gamma", "mu", "sigma", "ustar")}]


def flow_of(flow, i):
    """'cycle': the three call flows from step to step, against the noise modes' own cycle of three"""
    return FLOWS[(i + i // 3) % 3] if flow == "cycle" else flow


def noise_of(i):
    return NOISE[i % 3]


def problems(fam, p, n, J, dtype, which="R"):
    """(A, U0, [problem]) of a sequence.  R / S: one problem of ``cr.family``.  P: P0 diagonal; P1 a dense Sigma; P2 a dense
    Gamma; P3 ANOTHER dense Gamma of the same size; P4 only y, mu, ustar changed; P5 = P0."""
    d = cr.family(fam, p, n, J, dtype)
    keys = ("y", "Gamma", "mu", "sigma", "ustar")
    if which != "P":
        return d["A"], d["U0"], [{k: d[k] for k in keys}]
    out = []
    for k, (dg, ds) in enumerate(P_DENSE):
        q = cr.family(fam, p, n, J, dtype, dense_gamma=dg, dense_sigma=ds)
        q = {key: q[key] for key in keys}
        if k in (3, 4):
            q["Gamma"] = cr.family(fam, p, n, J, dtype, seed=p + n + J + 1, dense_gamma=True)["Gamma"]
        if k == 4:
            rng = np.random.default_rng(p + n + J + 2)
            q["y"] = q["y"] + 0.05 * rng.standard_normal(n)
            q["mu"] = q["mu"] + 0.1 * rng.standard_normal((p, 1))
            q["ustar"] = q["ustar"] + 0.1 * rng.standard_normal((p, 1))
        out.append(q)
    assert np.array_equal(out[0]["sigma"], out[5]["sigma"]) and not np.array_equal(out[2]["Gamma"], out[3]["Gamma"])
    return d["A"], d["U0"], out


def expected_form(eng_name, s, prob):
    """The update form ``pick`` names for a step (-1: aldi_constant, whose two launches carry no form)."""
    p, n, J, dtype = T_ENGINE if eng_name == "T" else ENGINES[eng_name]
    if s["update"] == "aldi_constant":
        return -1
    return ge.pick(p, n, J, dtype, s["update"], s["kw"]["time_step"], dense_sigma=not cr.is_diagonal(prob["sigma"]))[0]


def forward(A, Uh, dt):
    Z = A @ Uh
    return (GAIN * (Z + 0.05 * np.sin(Z))).astype(dt).astype(np.float64)


def params_of(eng_mod, s, idx):
    kw, t_prev = s["kw"], s["t_prev"]
    return eng_mod.step_params(update=s["update"], time_step=kw["time_step"], first_step=not t_prev, t_len=len(t_prev),
                               t_last=t_prev[-1] if t_prev else 0.0, delta_t=kw.get("delta_t"), spinup=kw.get("spinup", 4.0),
                               step_index=idx, T=30)


def ts_of(s):
    kw, t_prev = s["kw"], s["t_prev"]
    return dict(time_step=kw["time_step"], delta_t=kw.get("delta_t"), spinup=kw.get("spinup", 4.0), first_step=not t_prev,
                t_len=len(t_prev), t_last=t_prev[-1] if t_prev else 0.0)


def whole_step_ref(s, prob, Uh, Gh, xi_h):
    """Check 4's reference: (U_next, t, metrics) of oracle/ces_numpy.py from the step's own inputs."""
    p, J = Uh.shape
    st = oc.OracleState(p, Gh.shape[0], J, prob["mu"], prob["sigma"], prob["ustar"])
    st.metrics["t"] = list(s["t_prev"])
    st.trace_len = 1 if not s["t_prev"] else 2
    kw = {k: v for k, v in s["kw"].items() if k == "time_step" or v is not None}
    ref = oc.factored_step(st, prob["y"], Uh, Gh, prob["Gamma"], xi_h, update=s["update"], **kw)
    return ref, st


class Record:
    """Ratios of every comparison to its bar, by part; ``worst`` per part for the record a module prints when it ends."""

    def __init__(self):
        self.rows, self.worst, self.steps = [], {}, []

    def add(self, label, i, part, ratio, strict, detail=""):
        ratio = float(ratio)
        self.rows.append((label, i, part, ratio))
        w = self.worst.setdefault(part, [0.0, 0])
        w[0], w[1] = max(w[0], ratio if np.isfinite(ratio) else np.inf), w[1] + 1
        if strict:
            assert ratio <= 1.0, (label, "step %d" % i, part, "ratio to the bar %.4g" % ratio, detail)

    def at(self, label, i):
        return {part: r for lab, k, part, r in self.rows if lab == label and k == i}


def rel_max(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    if not np.all(np.isfinite(got)):
        return np.inf
    return float(np.max(np.abs(got - ref)) / max(np.max(np.abs(ref)), 1e-300))


def bound_ratio(dev, ref, B, c, eps, extra=0.0):
    """worst |dev - ref| / ((c eps + extra) B): the ``held`` of tests/test_gpu_calibrate_edges.py as a ratio to its bar"""
    dev, ref, B = (np.asarray(a, dtype=np.float64) for a in (dev, ref, B))
    if dev.shape != ref.shape or not np.all(np.isfinite(dev)):
        return np.inf
    err = np.abs(dev - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(B > 0, err / ((c * eps + extra) * B), np.where(err > 0, np.inf, 0.0))
    return float(r.max())


def run_sequence(eng_mod, eng, A, U0, probs, steps, flow, rec, label, forms=None, strict=True, between=None, host_noise=False,
                 before_result=None):
    """Drive ``eng`` through ``steps`` (tables above) under ``flow`` ('step' | 'split' | 'sharded' | 'cycle') with checks 1-5
    after every step.  forms: the expected update form per step.  between: {i: f(eng)} run in front of step i (another stage on
    the same engine).  before_result: {i: f(eng)} run after step i has been launched and before its result is read, in every
    flow -- where ``calibrate._run_device`` has the forward map of U_new: the one place a stage call meets a deferred metric
    finalisation.  host_noise: the engine-drawn blocks restated by oracle/philox.py instead of read through cesx_draw_noise.
    Returns [(form, warm_inverse)] per step."""
    from ces_amd.dist import ShardedUpdate
    p, n, J = eng.p, eng.n_obs, eng.J
    ndt = eng.np_dtype
    dtype = ndt.name
    eps = cr.eps_of(dtype)
    rng = np.random.default_rng([SEED, p, n, J])
    bufs = [guarded(eng, rows) for rows in (p, n, p, p, p)]
    (U, G, xi), outs = [v for _, v in bufs[:3]], [v for _, v in bufs[3:]]
    put(U, U0.astype(ndt))
    sh = ShardedUpdate(eng)
    sh._recentered = True            # the TABLE says which steps recentre: the driver's own "first call recentres" would turn the
    #                                  cycling flow's first sharded step (2, on the predicted shift) into a recentred one
    #                                  unseen; a step without a valid shift is an error of the engine (CESX_ESTATE), not a pass
    log, prev = [], None
    for i, s in enumerate(steps):
        prob, upd, fl, noise, idx = probs[s["prob"]], s["update"], flow_of(flow, i), noise_of(i), STEP0 + i
        if between and i in between:
            between[i](eng)
        eng.set_problem(prob["y"], prob["Gamma"], prob["mu"], prob["sigma"], prob["ustar"])
        if prev is not None:
            U.copy_(prev)
        if s["edit"]:
            U.mul_(1.03125)                       # the caller rescales the ensemble in place: a fresh centring pass is due
        Uh = U.cpu().numpy().astype(np.float64)
        Gh = forward(A, Uh, ndt)
        put(G, Gh.astype(ndt))
        prm = params_of(eng_mod, s, idx)
        if noise == "injected":
            xi_h = rng.standard_normal((p, J)).astype(ndt).astype(np.float64)
            put(xi, xi_h.astype(ndt))
            xi_t = xi
        else:
            xi_t = None
            xi_h = (philox.noise_block(p, J, SEED, idx, dtype=ndt).astype(ndt).astype(np.float64) if host_noise
                    else eng.draw_noise(idx).cpu().numpy().astype(np.float64))
        out = outs[i % 2]
        dg = not cr.is_diagonal(prob["Gamma"])
        cu = cr.c_update(p, n, dense_gamma=dg)
        lab = "%s %d %s/%s %s %s" % (label, i, upd, s["rule"], fl, noise)
        ahead = noise == "ahead"
        if upd == "aldi_constant":
            # both passes through the split entry points in every flow, so that the drift can be read between them
            if fl == "sharded":
                mom = sh.begin(prm, U, G, recenter=s["recenter"], noise_step=idx if ahead else None)
            else:
                if s["recenter"]:
                    eng.set_shift(eng.colsum(U, G))
                if ahead:
                    eng.prefetch_noise(idx)
                mom = eng.moments(U, G)
            absmax = eng.apply_drift(prm, mom, U, G, out)
            drift = out.cpu().numpy().astype(np.float64)
            dd = eng.debug_dense()
            ref, B = cr.update_ref("drift", dd, None, Uh, Gh, None, prob, J=J)
            rec.add(label, i, "K3 drift", bound_ratio(drift, ref, B, cu, eps), strict, lab)
            rec.add(label, i, "K3 max|drift|", 0.0 if float(absmax.cpu()[0]) == np.max(np.abs(drift)) else np.inf, strict, lab)
            eng.apply_finish(prm, absmax, U, xi_t, out)
            if before_result and i in before_result:
                before_result[i](eng)
            res = eng.result()
            got = out.cpu().numpy().astype(np.float64)
            hk_ref = 0.1 / np.max(np.abs(drift))
            rec.add(label, i, "K2 hk", abs(res.hk - hk_ref) / (1e-15 * hk_ref), strict, lab)
            ref, B = cr.update_ref("finish", dd, res.hk, Uh, None, xi_h, prob, J=J, drift=drift)
            rec.add(label, i, "K3 finish", bound_ratio(got, ref, B, cu, eps), strict, lab)
            form = -1
        else:
            if fl == "step":
                eng.step(prm, U, G, xi=xi_t, out=out, recenter=s["recenter"])
            elif fl == "split":
                if s["recenter"]:
                    eng.set_shift(eng.colsum(U, G))
                if ahead:
                    eng.prefetch_noise(idx)
                mom = eng.moments(U, G)
                eng.apply(prm, mom, U, G, xi_t, out=out)
            else:
                sh.begin(prm, U, G, recenter=s["recenter"], noise_step=idx if ahead else None)
                sh.finish(prm, U, G, xi=xi_t, out=out)
            if before_result and i in before_result:
                before_result[i](eng)
            res = sh.result() if fl == "sharded" else eng.result()
            got = out.cpu().numpy().astype(np.float64)
            form = eng.update_form()
            if forms is not None:
                rec.add(label, i, "update form", 0.0 if form == forms[i] else np.inf, strict, (lab, form, forms[i]))
            dd = eng.debug_dense()
            kform = "eks" if upd == "eks" else cr.FORM_OF_UPDATE_FORM[form]
            ref, B = cr.update_ref(kform, dd, res.hk, Uh, Gh, xi_h, prob, J=J)
            rec.add(label, i, "K3 " + kform, bound_ratio(got, ref, B, cu, eps, extra=cr.BAND if kform == "eks" else 0.0), strict, lab)
        log.append((form, eng.warm_inverse()))
        # 2. K2 from the step's own inputs
        bar = K2_BAR[dtype]
        k2 = cr.dense_from_inputs(Uh, Gh, prob, upd, dtype, **({} if upd == "aldi_constant" else ts_of(s)))
        for key in ("ubar", "gbar", "C", "K", "M"):
            rec.add(label, i, "K2 " + key, rel_max(dd[key], k2[key]) / bar, strict, lab)
        try:
            Lref = np.linalg.cholesky(dd["C"])
            rec.add(label, i, "K2 L", rel_max(np.tril(dd["L"]), Lref) / cr.BAND, strict, lab)
        except np.linalg.LinAlgError:
            rec.add(label, i, "K2 L", np.inf, strict, lab)
        scal = [("bias", res.bias), ("self_bias", res.self_bias)]
        if upd != "aldi_constant":
            scal += [("hk", res.hk), ("t", res.t_new)]
            if s["kw"]["time_step"] == "spectral":
                scal.append(("radspec", res.radspec))
        else:
            rec.add(label, i, "K2 t", abs(res.t_new - (res.hk + s["t_prev"][-1])) / (1e-15 * res.t_new), strict, lab)
        for key, val in scal:
            rec.add(label, i, "K2 " + key, abs(val - k2[key]) / abs(k2[key]) / bar, strict, (lab, val, k2[key]))
        # 3. the data metrics
        Lg, Li = cr.whitening(prob["Gamma"])
        if Lg is None:
            m = cr.data_metrics_ref(Gh, dd["gbar"], prob["y"], 1.0 / np.diag(prob["Gamma"]))
        else:
            m = cr.data_metrics_ref(Li @ Gh, Li @ dd["gbar"], Li @ prob["y"], np.ones(n), G_abs=np.abs(Li) @ np.abs(Gh))
        cm = cr.c_metric(n, dense_gamma=dg)
        for key in ("bias_data", "self_bias_data"):
            val, scale = m[key]
            rec.add(label, i, "metrics " + key, abs(getattr(res, key) - val) / (cm * eps * scale), strict, lab)
        # 4. the whole step
        ref, st = whole_step_ref(s, prob, Uh, Gh, xi_h)
        rec.add(label, i, "whole U_next", rel_max(got, ref) / TOL[dtype], strict, lab)
        rec.add(label, i, "whole t", abs(res.t_new - st.metrics["t"][-1]) / abs(st.metrics["t"][-1]) / TOL[dtype], strict, lab)
        # 5. in-place use
        same = np.array_equal(U.cpu().numpy().astype(np.float64), Uh) and np.array_equal(G.cpu().numpy().astype(np.float64), Gh)
        rec.add(label, i, "inputs unchanged", 0.0 if same else np.inf, strict, lab)
        rec.add(label, i, "guards", 0.0 if all(guards_intact(f, v) for f, v in bufs) else np.inf, strict, lab)
        prev = out
    return log


def run_pipelined(eng_mod, eng, A, U0, probs, steps, rec, label, pipelined, strict=True):
    """The sequence through ShardedUpdate.begin / finish: ``finish(i)``, ``begin(i + 1)`` given step i + 1's own rule,
    ``result(i)`` -- or, not pipelined, ``result(i)`` first.  The buffers of a step stay untouched until its result has been read
    (include/cesx.h), so the input of step i + 1 is the output tensor of step i itself and G, xi alternate between two tensors.
    cesx_debug_dense mixes two steps here: per step only check 4 applies.  Returns [(U_next, step result)] for the bit
    comparison of the two orders."""
    from ces_amd.dist import ShardedUpdate
    p, n, J = eng.p, eng.n_obs, eng.J
    ndt = eng.np_dtype
    dtype = ndt.name
    rng = np.random.default_rng([SEED, p, n, J])
    Us, Gs, xis = [eng.empty(p) for _ in range(3)], [eng.empty(n) for _ in range(2)], [eng.empty(p) for _ in range(2)]
    put(Us[2], U0.astype(ndt))
    sh = ShardedUpdate(eng)
    prob = probs[0]
    eng.set_problem(prob["y"], prob["Gamma"], prob["mu"], prob["sigma"], prob["ustar"])
    prms = [params_of(eng_mod, s, STEP0 + i) for i, s in enumerate(steps)]

    def stage(i, U):
        """the inputs of step i on the device and on the host; its ``begin``"""
        Uh = U.cpu().numpy().astype(np.float64)
        Gh = forward(A, Uh, ndt)
        put(Gs[i % 2], Gh.astype(ndt))
        if noise_of(i) == "injected":
            xi_h = rng.standard_normal((p, J)).astype(ndt).astype(np.float64)
            put(xis[i % 2], xi_h.astype(ndt))
            xi_t = xis[i % 2]
        else:
            xi_t, xi_h = None, philox.noise_block(p, J, SEED, STEP0 + i, dtype=ndt).astype(ndt).astype(np.float64)
        sh.begin(prms[i], U, Gs[i % 2], recenter=steps[i]["recenter"], noise_step=STEP0 + i if noise_of(i) == "ahead" else None)
        return dict(U=U, G=Gs[i % 2], xi=xi_t, Uh=Uh, Gh=Gh, xi_h=xi_h)

    out_rows = []
    cur = stage(0, Us[2])
    for i, s in enumerate(steps):
        out = sh.finish(prms[i], cur["U"], cur["G"], xi=cur["xi"], out=Us[i % 2])
        nxt = None
        if pipelined and i + 1 < len(steps):
            nxt = stage(i + 1, out)
        res = sh.result()
        got = out.cpu().numpy()
        ref, st = whole_step_ref(s, prob, cur["Uh"], cur["Gh"], cur["xi_h"])
        rec.add(label, i, "whole U_next", rel_max(got, ref) / TOL[dtype], strict, label)
        rec.add(label, i, "whole t", abs(res.t_new - st.metrics["t"][-1]) / abs(st.metrics["t"][-1]) / TOL[dtype], strict, label)
        out_rows.append((got.copy(), np.array([res.hk, res.t_new, res.self_bias, res.self_bias_data, res.bias_data, res.bias,
                                             res.radspec if s["kw"]["time_step"] == "spectral" else 0.0])))
        if not pipelined and i + 1 < len(steps):
            nxt = stage(i + 1, out)
        cur = nxt
    return out_rows
