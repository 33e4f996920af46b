"""The staged references of oracle/calibrate_ref.py against what is already pinned, and the elementwise bar against itself, so
that neither a wrong reference nor a bound too loose to see anything can pass a wrong kernel.

1. moments_ref -> dense_ref -> update_ref chained together reproduce every step case the REAL reference produced
   (tests/golden/steps_*.npz) at the bar tests/test_oracle_golden.py holds oracle/ces_numpy.py to, and all K3 forms agree in fp64.
2. On every K3 case of tests/test_gpu_calibrate_edges.py, with that case's own generated inputs and in both problem families:
   (a) the unmutated form evaluated by numpy IN THE ENGINE DTYPE stays below c eps B (fp64 cases: fp64 against an extended
       precision evaluation);
   (b) every mutant of calibrate_ref.mutants the case's form contains exceeds 4 c eps B in at least one entry in at least one
       of the two families (the GPU test runs every case in both).
   K3 is independent from column to column, so (b) is evaluated on the first and the last 128 particles of a large case (a
   mutant seen there is seen in the whole).  (a) runs over all particles in fp32; an fp64 case with J > 256 takes every
   fourth of those 256 columns (its reference is numpy's extended precision, which has no BLAS behind it).
3. The same two conditions for K1 on every case of the Gram table: numpy in the engine dtype, summed slab by slab, stays
   inside c_gram eps scale; the last particle dropped, the last J tile dropped and a padding column summed each leave 4x it."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import rel_err, step_case  # noqa: E402
import test_gpu_calibrate_edges as ge  # noqa: E402

from oracle import calibrate_ref as cr  # noqa: E402

TOL_STAGED = 1e-9                # tests/test_oracle_golden.py, TOL_FACTORED


def host_dense(d, update, J, **ts):
    """K1 and K2 on the host in fp64: what the device's debug_dense and hk stand for in the GPU test."""
    p = d["U0"].shape[0]
    Lg, Li = cr.whitening(d["Gamma"])
    Gw = d["G"] if Lg is None else Li @ d["G"]
    sums = np.concatenate([[float(J)], d["U0"].sum(axis=1), Gw.sum(axis=1)])
    shift = cr.round_shift(sums, np.float64)
    mom, _ = cr.moments_ref(d["U0"], Gw, shift[:p], shift[p:])
    return cr.dense_ref(mom, shift, d, update, **ts), Gw, Li


# ---- 1. the staged references reproduce the real reference's steps ----------------------------------------------------------

def test_staged_references_reproduce_the_golden_steps(manifest, golden_steps):
    assert len(manifest["steps"]) >= 100
    for case in manifest["steps"]:
        c = step_case(golden_steps, case)
        p, n, J, upd, kw = case["p"], case["n_obs"], case["J"], case["update"], case["kwargs"]
        d = dict(y=c["y"], Gamma=c["Gamma"], mu=c["mu"], sigma=c["sigma"], ustar=c["ustar"], U0=c["U0"], G=c["G"], xi=c["xi"])
        t_prev = list(case["t_prev"])
        ts = dict(time_step=kw.get("time_step"), delta_t=kw.get("delta_t"), spinup=kw.get("spinup", 4.0),
                  first_step=case["trace_len"] == 1, t_len=len(t_prev), t_last=t_prev[-1] if t_prev else 0.0)
        dd, Gw, Li = host_dense(d, upd, J, **(ts if upd != "aldi_constant" else {}))
        if upd == "aldi":
            outs = [cr.update_ref(form, dd, dd["hk"], d["U0"], d["G"], d["xi"], d, J=J)[0] for form in ("assembled", "hkfree", "chained")]
            for o in outs[1:]:
                assert rel_err(o, outs[0]) < 1e-12, (case["id"], "the K3 forms disagree")
            Uk, t_new = outs[0], dd["t"]
        elif upd == "eks":
            Uk, t_new = cr.update_ref("eks", dd, dd["hk"], d["U0"], d["G"], d["xi"], d, J=J)[0], dd["t"]
        else:
            drift = cr.update_ref("drift", dd, None, d["U0"], d["G"], None, d, J=J, switch=kw.get("switch", 1.0))[0]
            hk = 0.1 / np.max(np.abs(drift))
            t_new = hk if case["trace_len"] == 1 else hk + t_prev[-1]
            Uk = cr.update_ref("finish", dd, hk, d["U0"], None, d["xi"], d, J=J, drift=drift)[0]
        assert rel_err(Uk, c["Uk"]) < TOL_STAGED, (case["id"], upd, rel_err(Uk, c["Uk"]))
        assert abs(t_new - float(c["t_new"])) <= TOL_STAGED * max(1.0, abs(float(c["t_new"])))
        if Li is None:
            m = cr.data_metrics_ref(d["G"], dd["gbar"], d["y"], 1.0 / np.diag(d["Gamma"]))
        else:                       # a dense Gamma: the quadratic forms in the whitened coordinates the engine works in
            m = cr.data_metrics_ref(Gw, Li @ dd["gbar"], Li @ d["y"], np.ones(n))
        got = np.array([dd["self_bias"], m["self_bias_data"][0], m["bias_data"][0], dd["bias"]])
        assert np.allclose(got, c["metrics"], rtol=TOL_STAGED, atol=0), (case["id"], got, c["metrics"])
        if kw.get("time_step") == "spectral":
            assert np.allclose(dd["radspec"], c["radspec"], rtol=1e-8)


def test_moments_reference_layout_and_scale():
    """The packed buffer has the layout of include/cesx.h, and its scale bounds it entry by entry."""
    rng = np.random.default_rng(3)
    p, n, J = 5, 3, 40
    U, G = rng.standard_normal((p, J)) + 2.0, rng.standard_normal((n, J)) - 1.0
    su, sg = U.mean(axis=1), G.mean(axis=1)
    mom, scale = cr.moments_ref(U, G, su, sg)
    o = cr.moments_layout(p, n)
    assert len(mom) == o["tail"] and o["len"] == 1 + p + p * p + n + p * n + n * n + 2 and mom[0] == J
    m = cr.unpack(np.concatenate([mom, [0.0, 0.0]]), p, n)
    assert np.allclose(m["Saa"] / (J - 1), np.cov(U)) and np.allclose(m["Sab"] / (J - 1), np.cov(U, G)[:p, p:])
    assert np.allclose(m["Sbb"] / (J - 1), np.cov(G)) and np.all(np.abs(m["sa"]) < 1e-12 * J) and np.all(np.abs(mom[1:]) <= scale[1:] * (1 + 1e-12))
    assert np.array_equal(cr.round_shift([4.0, 1.0, 2.0], np.float32), np.array([0.25, 0.5]))
    assert cr.round_shift([3.0, 1.0], np.float32)[0] == float(np.float32(1.0 / 3.0)) != 1.0 / 3.0


# ---- 2. the bar: inside for the right form, outside for every mutant ------------------------------------------------------

def k3_shapes():
    """The K3 cases that differ in what the host conditions depend on (the noise source and the buffer offset do not)."""
    seen, out = set(), []
    for c in ge.K3_CASES:
        key = (c["p"], c["n"], c["J"], c["dtype"], c["update"], c["ts"], c["dg"], c["ds"], c["form"])
        if key not in seen:
            seen.add(key)
            out.append(c)
    return out


def launches(c, d, dd):
    """[(form, kwargs of update_ref / mutants)] of the launches a case compares."""
    J = c["J"]
    if c["update"] == "aldi_constant":
        drift = cr.update_ref("drift", dd, None, d["U0"], d["G"], None, d, J=J)[0]
        # (the device hands the second pass its drift rounded to the engine dtype; so does the GPU test)
        drift = drift.astype(np.dtype(c["dtype"])).astype(np.float64)
        hk = 0.1 / np.max(np.abs(drift))
        return [("drift", dict(hk=None, G=d["G"], xi=None)), ("finish", dict(hk=hk, G=None, xi=d["xi"], drift=drift))]
    form = "eks" if c["update"] == "eks" else cr.FORM_OF_UPDATE_FORM[c["form"]]
    return [(form, dict(hk=dd["hk"], G=d["G"], xi=d["xi"]))]


@pytest.mark.parametrize("c", k3_shapes(), ids=ge.k3_id)
def test_the_bound_holds_the_right_form_and_no_mutant(c):
    p, n, J, dtype = c["p"], c["n"], c["J"], c["dtype"]
    eps, cu = cr.eps_of(dtype), cr.c_update(p, n, dense_gamma=c["dg"])
    sub = np.arange(J) if J <= 256 else np.r_[0:128, J - 128:J]
    seen, reach = {}, {}
    for fam in cr.FAMILIES:
        d = ge.problem_of(c, fam)
        dd, _, _ = host_dense(d, c["update"], J, **(dict(time_step=c["ts"]) if c["update"] != "aldi_constant" else {}))
        for form, a in launches(c, d, dd):
            hk, drift = a["hk"], a.get("drift")
            extra = cr.BAND if form == "eks" else 0.0
            # (a) the right form in the engine dtype stays inside the bound, every entry
            if dtype == "float32":
                ref, B = cr.update_ref(form, dd, hk, d["U0"], a["G"], a["xi"], d, J=J, drift=drift)
                got = cr.update_in_dtype(form, dd, hk, d["U0"], a["G"], a["xi"], d, dtype, J=J, drift=drift)
            else:
                cols = sub if J <= 256 else sub[::4]
                pick = lambda x: None if x is None else x[:, cols]                                   # noqa: E731
                args = (form, dd, hk, pick(d["U0"]), pick(a["G"]), pick(a["xi"]), d)
                ref = cr.update_in_dtype(*args, np.longdouble, J=J, drift=pick(drift))
                got = cr.update_in_dtype(*args, dtype, J=J, drift=pick(drift))
                B = cr.update_ref(*args, J=J, drift=pick(drift))[1]
            ratio = float(np.max(np.abs(got - ref) / (eps * B)))
            reach[(fam, form)] = ratio
            assert ratio <= cu + extra / eps, (ge.k3_id(c), fam, form, "numpy in the engine dtype leaves the bound", ratio, cu)
            assert np.all(B > 0)
            # (b) every mutant leaves 4x the bound somewhere, in one family at least
            pick = lambda x: None if x is None else x[:, sub]                                        # noqa: E731
            Us, Gs, Xs, Ds = pick(d["U0"]), pick(a["G"]), pick(a["xi"]), pick(drift)
            ref, B = cr.update_ref(form, dd, hk, Us, Gs, Xs, d, J=J, drift=Ds)
            for name, mut in cr.mutants(form, dd, hk, Us, Gs, Xs, d, J=J, drift=Ds).items():
                r = float(np.max(np.abs(mut - ref) / ((cu * eps + extra) * B)))
                seen[(form, name)] = max(seen.get((form, name), 0.0), r)
    missed = {k: v for k, v in seen.items() if not v > 4.0}
    print("%s: numpy in the engine dtype reaches %s of c = %d; weakest mutant %s" % (
        ge.k3_id(c), {k: "%.3g" % v for k, v in reach.items()}, cu, min(seen.items(), key=lambda kv: kv[1])))
    assert len(seen) >= 8 and not missed, (ge.k3_id(c), "mutants the bound cannot see (ratio to the bound)", missed)


# ---- 3. K1: inside for the right sums, outside for a lost or a phantom particle -------------------------------------------

def k1_inputs(c):
    """U, G and the shift of a K1 case as tests/test_gpu_calibrate_edges.py::test_gram_kernels_at_their_edges makes them."""
    d = cr.family("data", c["p"], c["n"], c["J"], c["dtype"])
    rd = lambda a: a.astype(np.dtype(c["dtype"])).astype(np.float64)                                  # noqa: E731
    if c["far"]:
        U = rd(d["U0"] - d["U0"].mean(axis=1, keepdims=True) + 100.0 * d["U0"].std(axis=1, keepdims=True))
        G = rd(d["G"] - d["G"].mean(axis=1, keepdims=True) + 100.0 * d["G"].std(axis=1, keepdims=True))
        return U, G, np.zeros(c["p"] + c["n"])
    sums = np.concatenate([[float(c["J"])], d["U0"].sum(axis=1), d["G"].sum(axis=1)])
    return d["U0"], d["G"], cr.round_shift(sums, c["dtype"])


@pytest.mark.parametrize("c", ge.K1_CASES, ids=ge.k1_id)
def test_the_gram_bound_holds_the_right_sums_and_no_mutant(c):
    p, n, J, dtype = c["p"], c["n"], c["J"], c["dtype"]
    kt = 32 if dtype == "float32" else 16
    eps = cr.eps_of(dtype)
    chain = cr.gram_chain(p, n, J, dtype, 256, ge.gram_plan(p, n, J, dtype))
    cg = cr.c_gram(chain)
    U, G, shift = k1_inputs(c)
    ref, scale = cr.moments_ref(U, G, shift[:p], shift[p:])
    if dtype == "float32":
        got = cr.moments_in_dtype(U, G, shift[:p], shift[p:], dtype, chain)
        ratio = float(np.max(np.abs(got - ref)[1:] / (eps * scale[1:])))
        assert ratio <= cg, (ge.k1_id(c), "numpy in the engine dtype leaves the bound", ratio, cg)
    seen = {}
    for name, mut in cr.moments_mutants(U, G, shift[:p], shift[p:], kt).items():
        seen[name] = float(np.max(np.abs(mut - ref)[1:] / (cg * eps * scale[1:])))
    if c["far"]:
        seen.pop("padding_column_summed")          # (no shift at all: a zero column adds nothing, and nothing is wrong with that)
    print("%s: chain %d, c = %d; mutants / bound %s" % (ge.k1_id(c), chain, cg, {k: "%.3g" % v for k, v in seen.items()}))
    assert all(v > 4.0 for v in seen.values()), (ge.k1_id(c), "mutants the bound cannot see (ratio to the bound)", seen)


def test_the_mutants_named_in_the_design_exist():
    c = next(c for c in ge.K3_CASES if c["kernel"] == "update4")
    d = ge.problem_of(c, "prior")
    dd, _, _ = host_dense(d, "aldi", c["J"])
    cols = np.r_[0:8, c["J"] - 8:c["J"]]
    names = set(cr.mutants("chained", dd, dd["hk"], d["U0"][:, cols], d["G"][:, cols], d["xi"][:, cols], d, J=c["J"]))
    want = {"prior_dropped", "mu_dropped", "sigma_inv_last_entry_1pct", "alpha_zero", "noise_5pct", "last_1_particles_not_updated",
            "last_4_particles_not_updated"} | {"%s_%s" % (b, w) for b in ("L", "N", "K") for w in ("last_row", "last_col", "last_ktile")}
    assert names == want
    assert set(cr.mutants("hkfree", dd, dd["hk"], d["U0"][:, cols], d["G"][:, cols], d["xi"][:, cols], d, J=c["J"])) == \
        {w.replace("N_", "M_") for w in want}


def test_data_metric_reference_and_its_scale():
    rng = np.random.default_rng(5)
    n, J = 7, 33
    G, y = rng.standard_normal((n, J)), rng.standard_normal(n)
    gw = 1.0 / (0.5 + rng.random(n))
    gbar = G.mean(axis=1)
    m = cr.data_metrics_ref(G, gbar, y, gw)
    R, E = G - y[:, None], G - gbar[:, None]
    assert m["bias_data"][0] == pytest.approx(float((np.diag(R.T @ np.diag(gw) @ R) ** 2).mean()), rel=1e-13)
    assert m["self_bias_data"][0] == pytest.approx(float((np.diag(E.T @ np.diag(gw) @ E) ** 2).mean()), rel=1e-13)
    assert all(v[1] >= v[0] > 0 for v in m.values())
    # numpy in fp32, the way the kernels sum it, stays inside c_metric eps scale
    f = np.float32
    q = (gw.astype(f)[:, None] * (G.astype(f) - y.astype(f)[:, None]) ** 2).sum(axis=0, dtype=f).astype(np.float64)
    G32 = G.astype(f).astype(np.float64)
    m32 = cr.data_metrics_ref(G32, gbar, y, gw)
    assert abs(float((q * q).mean()) - m32["bias_data"][0]) <= cr.c_metric(n) * cr.EPS["float32"] * m32["bias_data"][1]
