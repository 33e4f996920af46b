"""The streaming chain summaries on the device (cesx_chain_summary_*, kernels_chainsum.hip; MCMC(..., chains=M, summary=True)).

Engine level: synthetic traces are uploaded and summed in three chunkings; every raw sum and half-chain output is held
elementwise to  c 2^-52 B  against the fp64 reference computed from the same, already rounded, trace
(tests/chain_summary_cases.py: the reference, the tables, the derivation of every c; tests/test_chain_summary_host.py shows
that the bounds see the reference made wrong).  Two identical runs are the same bits; the per-chain outputs are the same bits
across the chunkings, the pooled sums stay inside the bound in each.  A second table (``cs.PLAN_SHAPES``) holds the same
conditions at the launch plan's other regimes: several super tiles, several staged tiles a draw, more slabs than reduce
lanes, several slices and workgroups of the two row reduces.
Sampler level: every run twice with the same seed, with and without ``summary=True``: the chains are the same bits, and
``summary`` is the reference applied to the twin's kept states.

Measured on an MI355X (worst ratio of |device - reference| to its bound over the whole engine-level table):
NOTEBOOK.md, "Streaming chain summaries"."""
import os
import sys

import numpy as np
import pytest
from scipy import stats

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chain_summary_cases as cs  # noqa: E402
import map_cases as mc_  # noqa: E402
from test_emulate_host import gold_call, gold_prior, gold_problem, load_gold  # noqa: E402

pytestmark = pytest.mark.gpu
RAW = ("s1", "cc", "half_mean", "half_var", "within", "between")
PER_CHAIN = ("half_mean", "half_var")


def _ratio(got, ref, bound):
    """max |got - ref| / bound; an entry whose bound is 0 must be met exactly."""
    err = np.abs(np.asarray(got) - ref)
    zero = bound == 0
    assert np.all(err[zero] == 0), "an entry with a zero bound differs"
    return float(np.max(err[~zero] / bound[~zero])) if np.any(~zero) else 0.0


def _summed(eng, t, chunks, halves=True):
    eng.chain_summary_begin(t.shape[0])
    a = 0
    for k in chunks:
        eng.chain_summary_add(t[a:a + k] if k > 1 else t[a])          # (a single draw as a (p, J) state: U_dev itself)
        a += k
    return eng.chain_summary_read(halves=halves)


# ---- engine level -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("p", cs.P_SET)
def test_raw_sums_against_fp64(p, dtype):
    import torch
    from ces_amd import engine
    worst = {k: 0.0 for k in RAW + ("c",)}
    for J in cs.J_SET:
        eng = engine.Engine(p, 2, J, dtype=dtype)
        for N in cs.N_SET:
            for fam in cs.FAMILIES:
                x = cs.make_trace(p, J, N, fam, dtype)
                t = torch.as_tensor(x, device=eng.device).to(eng.torch_dtype).contiguous()
                assert np.array_equal(t.double().cpu().numpy(), x)          # the upload is exact: the trace was rounded first
                outs = {name: _summed(eng, t, ch) for name, ch in cs.chunkings(N).items()}
                again = _summed(eng, t, [N])
                ref = cs.ref_raw(x, c=outs["one"]["c"])
                bounds = cs.raw_bounds(ref)
                tag = (p, J, N, fam, dtype)
                # the pooled shift against the row mean of the first draw, then everything else about the device's own c
                mean0 = cs.ref_raw(x)["c"]
                worst["c"] = max(worst["c"], _ratio(outs["one"]["c"], mean0, cs.c_shift(J) * cs.EPS * ref["B_c"]))
                assert worst["c"] <= 1.0, tag
                for name, out in outs.items():
                    assert np.array_equal(out["c"], outs["one"]["c"]), tag
                    assert np.all(np.triu(out["cc"], 1) == 0), tag
                    for k in RAW:
                        r = _ratio(out[k], ref[k], bounds[k])
                        worst[k] = max(worst[k], r)
                        assert r <= 1.0, (tag, name, k, r)
                    for k in PER_CHAIN:                                  # a chain's sums do not depend on the chunking
                        assert np.array_equal(out[k], outs["one"][k]), (tag, name, k)
                for k in RAW + ("c",):                                   # two identical runs: the same bits
                    assert np.array_equal(again[k], outs["one"][k]), (tag, k)
                # the finalised dict of these sums against the reference's, inside the propagated bounds
                from ces_amd import sample
                fin, want, fb = sample.finalise_summary(outs["one"], N, J), cs.finalise_ref(ref), cs.summary_bounds(ref)
                for k, b in fb.items():
                    ok = np.isfinite(want[k]) & np.isfinite(b)
                    assert np.all(np.abs(fin[k] - want[k])[ok] <= b[ok]), (tag, k)
        eng.close()
    print("\n[chainsum] p = %d %s: worst |dev - ref| / bound %s" % (p, dtype, {k: "%.3g" % v for k, v in worst.items()}))


def _plan_cases():
    """(shape, dtype, families) over ``cs.PLAN_SHAPES``: both dtypes and both families, but (129, 5505, 4) -- whose extended
    precision reference takes seconds -- once per dtype with one family each."""
    out = []
    for shape in cs.PLAN_SHAPES:
        for k, dtype in enumerate(("float64", "float32")):
            out.append((shape, dtype, (cs.FAMILIES[k],) if shape == (129, 5505, 4) else cs.FAMILIES))
    return out


SINGLES_MAX = 1 << 16                                         # draw-by-draw adds too where N J p is at most this


@pytest.mark.parametrize("shape,dtype,families", _plan_cases(), ids=["p%d-J%d-N%d-%s" % (s + (d,)) for s, d, _ in _plan_cases()])
def test_raw_sums_at_the_plans_other_regimes(shape, dtype, families):
    """test_raw_sums_against_fp64 at the shapes that reach the launch plan's other regimes (``cs.PLAN_SHAPES``: several super
    tiles and the off-diagonal branch, two and three staged tiles a draw with a ragged last one, a second pass of the reduce
    lanes, several slices of the row sums -- their cap -- and several workgroups of the half reduce), under the same bounds:
    ``cs.raw_bounds``, ``cs.c_shift`` and ``cs.summary_bounds`` take their depths from the plan."""
    import torch
    from ces_amd import engine, sample
    p, J, N = shape
    worst = {k: 0.0 for k in RAW + ("c",)}
    eng = engine.Engine(p, 2, J, dtype=dtype)
    for fam in families:
        x = cs.make_trace(p, J, N, fam, dtype)
        t = torch.as_tensor(x, device=eng.device).to(eng.torch_dtype).contiguous()
        assert np.array_equal(t.double().cpu().numpy(), x)              # the upload is exact: the trace was rounded first
        chunkings = cs.chunkings(N)
        if N * J * p > SINGLES_MAX:
            del chunkings["singles"]
        outs = {name: _summed(eng, t, ch) for name, ch in chunkings.items()}
        again = _summed(eng, t, [N])
        ref = cs.ref_raw(x, c=outs["one"]["c"])
        bounds = cs.raw_bounds(ref)
        tag = (shape, fam, dtype)
        # the pooled shift against the row mean of the first draw, then everything else about the device's own c
        mean0 = np.asarray(x[0].astype(np.longdouble).sum(axis=1) / J, dtype=np.float64)
        worst["c"] = max(worst["c"], _ratio(outs["one"]["c"], mean0, cs.c_shift(J) * cs.EPS * ref["B_c"]))
        for name, out in outs.items():
            assert np.array_equal(out["c"], outs["one"]["c"]), tag
            assert np.all(np.triu(out["cc"], 1) == 0), tag
            for k in RAW:
                worst[k] = max(worst[k], _ratio(out[k], ref[k], bounds[k]))
            for k in PER_CHAIN:                                      # a chain's sums do not depend on the chunking
                assert np.array_equal(out[k], outs["one"][k]), (tag, name, k)
        for k in RAW + ("c",):                                       # two identical runs: the same bits
            assert np.array_equal(again[k], outs["one"][k]), (tag, k)
        print("\n[chainsum plan] %s %s %s %s: worst |dev - ref| / bound so far %s"
              % (shape, cs.plan_of(p, J), fam, dtype, {k: "%.3g" % v for k, v in worst.items()}))
        assert all(v <= 1.0 for v in worst.values()), (tag, worst)
        fin, want, fb = sample.finalise_summary(outs["one"], N, J), cs.finalise_ref(ref), cs.summary_bounds(ref)
        for k, b in fb.items():
            ok = np.isfinite(want[k]) & np.isfinite(b)
            assert np.all(np.abs(fin[k] - want[k])[ok] <= b[ok]), (tag, k)
    eng.close()


def test_error_returns_leave_the_stage_alone():
    import torch
    from ces_amd import engine
    p, J, N = 3, 65, 5
    eng = engine.Engine(p, 2, J, dtype="float64")
    x = cs.make_trace(p, J, N, "centred", "float64")
    t = torch.as_tensor(x, device=eng.device).contiguous()
    with pytest.raises(engine.CesxError) as exc:              # no begin yet
        eng.chain_summary_add(t[0])
    assert exc.value.code == engine.ESTATE
    with pytest.raises(engine.CesxError) as exc:
        eng.chain_summary_read()
    assert exc.value.code == engine.ESTATE
    for bad in (3, 0, -1):
        with pytest.raises(ValueError, match="n_draws must be >= 4"):
            eng.chain_summary_begin(bad)
    with pytest.raises(ValueError, match="chain_summary_add: trace must be"):
        eng.chain_summary_add(t[:, :, :-1])
    clean = _summed(eng, t, [2, 3])
    eng.chain_summary_begin(N)
    eng.chain_summary_add(t[:2])
    with pytest.raises(engine.CesxError) as exc:              # read before N draws
        eng.chain_summary_read()
    assert exc.value.code == engine.ESTATE and "fewer draws" in str(exc.value)
    with pytest.raises(engine.CesxError) as exc:              # add past N
        eng.chain_summary_add(t[:4])
    assert exc.value.code == engine.ESTATE and "more draws" in str(exc.value)
    eng.chain_summary_add(t[2:])                              # neither launched anything: the run goes on as if never asked
    out = eng.chain_summary_read(halves=True)
    for k in RAW + ("c",):
        assert np.array_equal(out[k], clean[k]), k
    with pytest.raises(engine.CesxError) as exc:              # complete: one more draw is past N
        eng.chain_summary_add(t[0])
    assert exc.value.code == engine.ESTATE
    # a new problem does not touch the stage
    eng.chain_summary_begin(N)
    eng.chain_summary_add(t[:2])
    eng.set_problem(np.zeros(2), np.eye(2), np.zeros(p), np.eye(p), np.zeros(p))
    eng.chain_summary_add(t[2:])
    out = eng.chain_summary_read(halves=True)
    for k in RAW + ("c",):
        assert np.array_equal(out[k], clean[k]), k
    eng.close()


# ---- sampler level ----------------------------------------------------------------------------------------------------------

M, N_MCMC, STRIDE, BURN = 130, 40, 3, 7
N_DRAWS = 11                                                  # steps 9, 12, .., 39


def _map_sampler(kind, noise):
    from ces_amd import calibrate, sample
    model, y, Gamma, mean, cov, _ = mc_.problem(kind, None)
    enka = calibrate.enka(2, 2, 130)
    enka.Ustar = mc_.start_ensemble(kind, 130, np.random.default_rng(4))
    s = sample.MCMC()
    s.mute_bar, s.y_obs, s.noise, s.trace_stride = True, y, noise, STRIDE
    prior = stats.multivariate_normal(mean=mean, cov=cov)
    return s, lambda n, **kw: s.model_mh(model, n, prior, enka, Gamma, chains=M, start="ensemble", delta=0.7, **kw)


def _gp_sampler(noise):
    from ces_amd import sample
    man, a = load_gold()
    c = [c for c in man["cases"] if c["name"] == "compounded_diag"][0]
    enka = gold_problem(a, c["scaled"])
    s = sample.MCMC()
    s.mute_bar, s.y_obs, s.noise, s.trace_stride, s.seed = True, a["prob_y"], noise, STRIDE, 77
    call, prior = gold_call(a, c["kwargs"]), gold_prior(a)
    return s, lambda n, **kw: s.gp_mh(enka, n, prior, chains=M, **dict(call, **kw))


def _check_summary(summary, twin_new, p):
    """``summary`` against the reference applied to the twin call's states ``twin_new`` (p, 1 + kept + 1, M): the state the
    call started from, its kept states and its off-stride last state."""
    draws = cs.draws_of(twin_new, N_MCMC, STRIDE, BURN)
    assert draws.shape == (N_DRAWS, p, M)
    ref = cs.ref_raw(draws)
    want, bounds = cs.finalise_ref(ref), cs.summary_bounds(ref)
    assert summary["n"] == N_DRAWS and summary["chains"] == M
    for k, b in bounds.items():
        assert summary[k].shape == want[k].shape and summary[k].dtype == np.float64
        assert np.all(np.abs(summary[k] - want[k]) <= b), (k, float(np.max(np.abs(summary[k] - want[k]) / b)))
    assert np.all(summary["rhat"] > 0.9) and np.all(summary["ess"] > 0) and np.all(summary["ess"] <= 2 * M * (N_DRAWS // 2))
    return ref


def _twins(make, fused, noise="device"):
    """The same call with and without summary=True, then a resumed second call of each."""
    import torch
    runs = []
    for summary in (False, True):
        s, call = make(noise)
        kw = dict(summary=True, burn=BURN) if summary else {}
        legs = []
        for leg in range(2):
            if noise == "numpy":
                np.random.seed(31 + leg)
            call(N_MCMC, fused=fused, **kw)
            legs.append(dict(samples=np.array(s.samples), dev=s.samples_device.clone(), accept=s.accept,
                             chains=np.array(s.accept_chains), launches=s.fused_launches, next=s._mh_next_step,
                             summary=getattr(s, "summary", None)))
        runs.append(legs)
    plain, summed = runs
    p = plain[0]["samples"].shape[0]
    kept = N_MCMC // STRIDE + 2                               # the start, 13 kept states, the off-stride last
    for leg in range(2):
        a, b = plain[leg], summed[leg]
        assert torch.equal(a["dev"], b["dev"]) and a["accept"] == b["accept"] and np.array_equal(a["chains"], b["chains"])
        assert a["launches"] == b["launches"] and (a["launches"] >= 1) == bool(fused) and a["next"] == b["next"] == N_MCMC * (leg + 1)
        assert a["summary"] is None
        assert a["samples"].shape == (p, kept + leg * (kept - 1), M) and b["samples"].shape == (p, 2 + leg, M)
        assert np.array_equal(b["samples"][:, -1, :], a["samples"][:, -1, :])          # the call's last state
        assert np.array_equal(b["samples"][:, 0, :], a["samples"][:, 0, :])            # the run's start state
        first = leg * (kept - 1)                              # a resumed call summarises its own draws
        _check_summary(b["summary"], a["samples"][:, first:, :], p)
    assert not np.array_equal(summed[0]["summary"]["mean"], summed[1]["summary"]["mean"])


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "steps"])
@pytest.mark.parametrize("kind", ["banana", "elliptic"])
def test_model_mh_summary_equals_the_twin(kind, fused):
    _twins(lambda noise: _map_sampler(kind, noise), fused)


@pytest.mark.parametrize("fused", [False, True], ids=["steps", "fused"])
def test_gp_mh_summary_equals_the_twin(fused):
    _twins(_gp_sampler, fused)


def test_step_path_with_numpy_noise():
    _twins(lambda noise: _map_sampler("banana", noise), False, noise="numpy")


def test_one_chain_keeps_the_reference_shape():
    """M = 1: ``samples`` is (p, 2) as the reference's (p, n_kept), and the summary is that of two half-chains."""
    from ces_amd import calibrate, sample
    model, y, Gamma, mean, cov, _ = mc_.problem("banana", None)
    enka = calibrate.enka(2, 2, 130)
    enka.Ustar = mc_.start_ensemble("banana", 130, np.random.default_rng(4))
    prior = stats.multivariate_normal(mean=mean, cov=cov)
    out = []
    for summary in (False, True):
        s = sample.MCMC()
        s.mute_bar, s.y_obs, s.noise = True, y, "device"
        s.model_mh(model, 30, prior, enka, Gamma, chains=1, delta=0.7, **(dict(summary=True) if summary else {}))
        out.append(s)
    plain, summed = out
    assert plain.samples.shape == (2, 31) and summed.samples.shape == (2, 2)
    assert np.array_equal(summed.samples[:, -1], plain.samples[:, -1]) and plain.accept == summed.accept
    ref = cs.ref_raw(plain.samples[:, 1:].T[:, :, None])
    want, bounds = cs.finalise_ref(ref), cs.summary_bounds(ref)
    assert summed.summary["n"] == 30 and summed.summary["chains"] == 1
    for k, b in bounds.items():
        assert np.all(np.abs(summed.summary[k] - want[k]) <= b), k
