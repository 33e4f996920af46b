"""The streaming marginals on the device (cesx_chain_hist_*, kernels_chainhist.hip; MCMC(..., chains=M, summary=True,
marginals=...)).

Engine level: synthetic traces are uploaded and counted; the reference is ``np.histogram`` / ``np.histogram2d`` with the
explicit edge arrays on the trace converted to fp64, per row and per pair.  Counts are integers: every comparison is
``np.array_equal``.  The traces are normal draws wider than the range with, planted into them, every edge, one ulp (of the
engine dtype) below and above every edge, +-inf and NaN; some rows have log-spaced edges.
Sampler level: the same seed run with ``summary=True`` alone, with ``marginals=`` as well, and with the full trace: the chains
and ``summary`` are the same bits, and ``marginals`` is numpy applied to the trace twin's kept states after ``burn``."""
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
COUNTS = ("hist1d", "below", "above", "hist2d", "outside2d")
# a slab of the launch plan is 256 chains at these sizes: 257 is one more; (65, 15617) takes slabs of 512 (two chains a lane)
J_SET = (1, 63, 65, 257, 513)
BINS = ((2, 2), (20, 20), (256, 64))
KEPT = (1, 3, 7)


def row_edges(r, bins):
    """Row r's edges: uniform, each row its own range; log-spaced for the rows with (r + bins) % 3 == 2."""
    if (r + bins) % 3 == 2:
        return np.geomspace(0.01, 3.0 + 0.25 * (r % 7), bins + 1)
    return np.linspace(-2.0 - 0.1 * (r % 5), 1.5 + 0.3 * (r % 4), bins + 1)


def make_edges(p, bins):
    return np.stack([row_edges(r, bins) for r in range(p)])


def make_pairs(p):
    if p < 2:
        return np.zeros((0, 2), dtype=np.int32)
    want = [(0, 1), (1, 0), (p - 1, 0), (p // 2, p - 1)]
    return np.array([q for k, q in enumerate(want) if q[0] != q[1] and q not in want[:k]], dtype=np.int32)


def make_trace(kept, p, J, dtype, e1, e2, seed):
    """(kept, p, J) in ``dtype``: normal draws of spread 2 (wider than every range), then per row the planted values, as many
    as fit, from an offset that moves with the row."""
    rng = np.random.default_rng(seed)
    dt = np.dtype(dtype)
    x = (2.0 * rng.standard_normal((kept, p, J))).astype(dt)
    for r in range(p):
        e = np.concatenate([e1[r], e2[r]]).astype(dt)
        plant = np.concatenate([e, np.nextafter(e, dt.type(-np.inf)), np.nextafter(e, dt.type(np.inf)),
                                np.array([np.inf, -np.inf, np.nan], dtype=dt)])
        n = min(plant.size, kept * J)
        at = rng.choice(kept * J, size=n, replace=False)
        take = (np.arange(n) + 7 * r) % plant.size
        flat = x[:, r, :].reshape(-1)
        flat[at] = plant[take]
        x[:, r, :] = flat.reshape(kept, J)
    return x


def numpy_counts(x, e1, e2, pairs):
    """The reference: np.histogram / np.histogram2d on the fp64 trace with the explicit edges."""
    x = np.asarray(x, dtype=np.float64)
    kept, p, J = x.shape
    out = dict(hist1d=np.zeros((p, e1.shape[1] - 1), dtype=np.int64), below=np.zeros(p, dtype=np.int64), above=np.zeros(p, dtype=np.int64),
               hist2d=np.zeros((len(pairs), e2.shape[1] - 1, e2.shape[1] - 1), dtype=np.int64), outside2d=np.zeros(len(pairs), dtype=np.int64))
    for r in range(p):
        v = x[:, r, :].ravel()
        out["hist1d"][r] = np.histogram(v, bins=e1[r])[0]
        out["below"][r] = np.count_nonzero(v < e1[r, 0])
        out["above"][r] = v.size - out["hist1d"][r].sum() - out["below"][r]
    for k, (i, j) in enumerate(pairs):
        h = np.histogram2d(x[:, i, :].ravel(), x[:, j, :].ravel(), bins=[e2[i], e2[j]])[0]
        assert np.array_equal(h, np.round(h))
        out["hist2d"][k] = h.astype(np.int64)
        out["outside2d"][k] = kept * J - out["hist2d"][k].sum()
    return out


def counted(eng, t, chunks, e1, e2, pairs, read_after=None):
    eng.chain_hist_begin(e1, e2, pairs)
    a, mid = 0, None
    for n, k in enumerate(chunks):
        eng.chain_hist_add(t[a:a + k] if k > 1 else t[a])            # (a single draw as a (p, J) state: U_dev itself)
        a += k
        if read_after == n:
            mid = eng.chain_hist_read()
    assert a == t.shape[0]
    return eng.chain_hist_read(), mid


def check_invariants(out, n_draws, J, pairs):
    assert all(out[k].dtype == np.int64 for k in COUNTS)
    assert np.array_equal(out["hist1d"].sum(axis=1) + out["below"] + out["above"], np.full(out["hist1d"].shape[0], n_draws * J))
    assert np.array_equal(out["hist2d"].sum(axis=(1, 2)) + out["outside2d"], np.full(len(pairs), n_draws * J))
    where = {tuple(q): k for k, q in enumerate(np.asarray(pairs).tolist())}
    for (i, j), k in where.items():
        if (j, i) in where:
            assert np.array_equal(out["hist2d"][where[(j, i)]], out["hist2d"][k].T)
            assert out["outside2d"][where[(j, i)]] == out["outside2d"][k]


# ---- engine level -----------------------------------------------------------------------------------------------------------

def run_shape(eng, p, J, dtype, seed):
    import torch
    pairs = make_pairs(p)
    for bins, bins2d in BINS:
        e1, e2 = make_edges(p, bins), make_edges(p, bins2d)
        for kept in KEPT:
            x = make_trace(kept, p, J, dtype, e1, e2, seed + 31 * bins + kept)
            t = torch.as_tensor(x, device=eng.device).contiguous()
            assert t.dtype == eng.torch_dtype
            ref = numpy_counts(x, e1, e2, pairs)
            tag = (p, J, dtype, bins, bins2d, kept)
            one, _ = counted(eng, t, [kept], e1, e2, pairs)
            for k in COUNTS:
                assert one[k].shape == ref[k].shape and np.array_equal(one[k], ref[k]), (tag, k)
            check_invariants(one, kept, J, pairs)
            if kept == 7:                                             # the same trace draw by draw and in uneven pieces
                single, _ = counted(eng, t, [1] * 7, e1, e2, pairs)
                pieces, mid = counted(eng, t, [2, 1, 4], e1, e2, pairs, read_after=1)
                ref_mid = numpy_counts(x[:3], e1, e2, pairs)
                for k in COUNTS:
                    assert np.array_equal(single[k], ref[k]) and np.array_equal(pieces[k], ref[k]), (tag, k)
                    assert np.array_equal(mid[k], ref_mid[k]), (tag, k, "the read in the middle")
                again = eng.chain_hist_read()                         # a second read: the same counts
                for k in COUNTS:
                    assert np.array_equal(again[k], ref[k]), (tag, k)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("p", [1, 5, 65])
def test_counts_equal_numpy(p, dtype):
    from ces_amd import engine
    for J in J_SET:
        eng = engine.Engine(p, 2, J, dtype=dtype)
        run_shape(eng, p, J, dtype, 1000 * p + J)
        eng.close()


def test_wide_slabs_draw_chunks_and_every_pair():
    """The launch plan's other paths: slabs of 512 chains (p = 65, J = 15 617: 17 row groups want 61 slabs), the draws cut into
    chunks over the grid's third axis (kept = 70 at a small shape: three chunks of 24), and 64 pairs at once."""
    import torch
    from ces_amd import engine
    p, J = 65, 15617
    eng = engine.Engine(p, 2, J, dtype="float32")
    e1, e2 = make_edges(p, 20), make_edges(p, 20)
    pairs = np.array([(i, (i + 1 + i % 3) % p) for i in range(64)], dtype=np.int32)
    x = make_trace(3, p, J, "float32", e1, e2, 5)
    out, _ = counted(eng, torch.as_tensor(x, device=eng.device), [3], e1, e2, pairs)
    ref = numpy_counts(x, e1, e2, pairs)
    for k in COUNTS:
        assert np.array_equal(out[k], ref[k]), k
    check_invariants(out, 3, J, pairs)
    eng.close()
    for p, J, kept in ((2, 65, 70), (5, 257, 131)):
        eng = engine.Engine(p, 2, J, dtype="float64")
        e1, e2, pairs = make_edges(p, 20), make_edges(p, 20), make_pairs(p)
        x = make_trace(kept, p, J, "float64", e1, e2, 6)
        out, _ = counted(eng, torch.as_tensor(x, device=eng.device), [kept], e1, e2, pairs)
        ref = numpy_counts(x, e1, e2, pairs)
        for k in COUNTS:
            assert np.array_equal(out[k], ref[k]), (p, J, kept, k)
        eng.close()


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_every_draw_in_one_bin(dtype):
    """Worst contention: every chain and draw in one bin gives that bin exactly J kept, all others 0 -- one draw per add (every
    lane of a wave adds to one LDS counter) and many (a lane's run of equal bins is added once)."""
    import torch
    from ces_amd import engine
    p, J = 3, 1000
    eng = engine.Engine(p, 2, J, dtype=dtype)
    e1, e2 = np.stack([np.linspace(-1.0, 1.0, 65)] * p), np.stack([np.linspace(-1.0, 1.0, 21)] * p)
    pairs = np.array([(0, 2), (2, 1)], dtype=np.int32)
    for kept in (1, 70):
        t = torch.full((kept, p, J), 0.3, dtype=eng.torch_dtype, device=eng.device)
        t[:, 1, :] = -0.95
        out, _ = counted(eng, t, [kept], e1, e2, pairs)
        want1 = np.zeros((p, 64), dtype=np.int64)
        for r, v in enumerate((0.3, -0.95, 0.3)):
            want1[r, np.searchsorted(e1[r], np.float64(t[0, r, 0].item()), side="right") - 1] = J * kept
        want2 = np.zeros((2, 20, 20), dtype=np.int64)
        k3, k95 = (np.searchsorted(e2[0], np.float64(t[0, r, 0].item()), side="right") - 1 for r in (0, 1))
        want2[0, k3, k3] = J * kept
        want2[1, k3, k95] = J * kept
        assert np.array_equal(out["hist1d"], want1) and np.array_equal(out["hist2d"], want2)
        assert not out["below"].any() and not out["above"].any() and not out["outside2d"].any()
        t[:] = 5.0                                                    # and every draw above the range
        out, _ = counted(eng, t, [kept], e1, e2, pairs)
        assert not out["hist1d"].any() and not out["hist2d"].any() and not out["below"].any()
        assert np.array_equal(out["above"], np.full(p, J * kept)) and np.array_equal(out["outside2d"], np.full(2, J * kept))
    eng.close()


def test_error_returns_leave_the_run_alone():
    import torch
    from ces_amd import engine
    p, J, kept = 3, 65, 5
    eng = engine.Engine(p, 2, J, dtype="float64")
    e1, e2, pairs = make_edges(p, 20), make_edges(p, 20), make_pairs(p)
    x = make_trace(kept, p, J, "float64", e1, e2, 9)
    t = torch.as_tensor(x, device=eng.device).contiguous()
    ref = numpy_counts(x, e1, e2, pairs)
    with pytest.raises(engine.CesxError) as exc:              # no begin yet
        eng.chain_hist_add(t[0])
    assert exc.value.code == engine.ESTATE and "cesx_chain_hist_begin has not been called" in str(exc.value)
    with pytest.raises(engine.CesxError) as exc:
        eng.chain_hist_read()
    assert exc.value.code == engine.ESTATE
    eng.chain_hist_begin(e1, e2, pairs)
    eng.chain_hist_add(t[:2])
    # every refusal from here on leaves the run in hand alone
    with pytest.raises(ValueError, match="chain_hist_add: trace must be"):
        eng.chain_hist_add(t[:, :, :-1])
    with pytest.raises(ValueError, match="chain_hist_add: trace must be"):
        eng.chain_hist_add(t.float())
    with pytest.raises(ValueError, match="chain_hist_add: trace must be"):
        eng.chain_hist_add(t[:, :2, :])
    lin = lambda n: np.stack([np.linspace(0.0, 1.0, n + 1)] * p)      # noqa: E731
    for bad1, bad2, badp, match in (
            (lin(1), e2, pairs, r"bins must be in \[2, 256\]"), (lin(257), e2, pairs, r"bins must be in \[2, 256\]"),
            (e1, lin(1), pairs, r"bins2d must be in \[2, 64\]"), (e1, lin(65), pairs, r"bins2d must be in \[2, 64\]"),
            (e1, e2, np.array([(0, 1)] * 65), r"n_pairs must be in \[0, 64\]"),
            (e1, e2, np.array([(1, 1)]), "two different rows"), (e1, e2, np.array([(0, p)]), "two different rows"),
            (e1, e2, np.array([(-1, 0)]), "two different rows"),
            (e1[:2], e2, pairs, "edges1 must have shape"), (e1, e2[:2], pairs, "edges2 must have shape"),
            (e1, None, pairs, "pairs need edges2")):
        with pytest.raises(ValueError, match=match):
            eng.chain_hist_begin(bad1, bad2, badp)
    for row, col, v in ((1, 3, np.nan), (2, 0, -np.inf), (0, 20, np.inf), (1, 4, e1[1, 3]), (1, 4, e1[1, 2])):
        bad = e1.copy()
        bad[row, col] = v
        with pytest.raises(ValueError, match="edges1 of row %d are not finite and strictly increasing" % row):
            eng.chain_hist_begin(bad, e2, pairs)
        bad = e2.copy()
        bad[row, col] = v
        if row in pairs:
            with pytest.raises(ValueError, match="edges2 of row %d are not finite and strictly increasing" % row):
                eng.chain_hist_begin(e1, bad, pairs)
    bad = e2.copy()
    bad[1] = np.nan                                           # a row no pair names is not read
    only02 = np.array([(0, 2)], dtype=np.int32)
    eng.chain_hist_add(t[2:])                                 # the run went on unharmed
    out = eng.chain_hist_read()
    for k in COUNTS:
        assert np.array_equal(out[k], ref[k]), k
    out, _ = counted(eng, t, [kept], e1, bad, only02)
    want = numpy_counts(x, e1, e2, only02)
    for k in COUNTS:
        assert np.array_equal(out[k], want[k]), k
    # a new problem does not touch the stage, and no pairs at all is a run too
    eng.chain_hist_begin(e1)
    eng.chain_hist_add(t[:2])
    eng.set_problem(np.zeros(2), np.eye(2), np.zeros(p), np.eye(p), np.zeros(p))
    eng.chain_hist_add(t[2:])
    out = eng.chain_hist_read()
    assert np.array_equal(out["hist1d"], ref["hist1d"]) and out["hist2d"].shape == (0, 2, 2) and out["outside2d"].shape == (0,)
    eng.close()


def test_a_sharded_engine_is_refused():
    """J_local != J_global: the stage would count its shard alone, so begin refuses (CESX_EINVAL) and nothing is started; the
    same descriptor on an unsharded engine of the same shape runs, and a run in hand there is not disturbed by a refusal."""
    import torch
    from ces_amd import engine
    p, J, kept = 3, 65, 3
    e1, e2, pairs = make_edges(p, 20), make_edges(p, 20), make_pairs(p)
    x = make_trace(kept, p, J, "float64", e1, e2, 12)
    for Jg, off in ((2 * J, 0), (2 * J, J), (J + 1, 1)):
        eng = engine.Engine(p, 2, J, dtype="float64", J_global=Jg, j_offset=off)
        t = torch.as_tensor(x, device=eng.device).contiguous()
        for args in ((e1, e2, pairs), (e1,)):
            with pytest.raises(ValueError, match="sharded chains"):
                eng.chain_hist_begin(*args)
        with pytest.raises(engine.CesxError) as exc:          # nothing was started
            eng.chain_hist_add(t)
        assert exc.value.code == engine.ESTATE and "cesx_chain_hist_begin has not been called" in str(exc.value)
        with pytest.raises(engine.CesxError) as exc:
            eng.chain_hist_read()
        assert exc.value.code == engine.ESTATE
        eng.close()
    eng = engine.Engine(p, 2, J, dtype="float64", J_global=J)      # J_global given and equal: not sharded
    out, _ = counted(eng, torch.as_tensor(x, device=eng.device).contiguous(), [kept], e1, e2, pairs)
    ref = numpy_counts(x, e1, e2, pairs)
    for k in COUNTS:
        assert np.array_equal(out[k], ref[k]), k
    eng.close()


# ---- sampler level ----------------------------------------------------------------------------------------------------------

M, N_MCMC, STRIDE, BURN = 96, 40, 3, 7
N_DRAWS = 11                                                  # steps 9, 12, .., 39
MARG = dict(bins=24, bins2d=20, pairs=[(0, 1), (1, 0)], width=4.0)
SUMMARY_KEYS = ("mean", "cov", "within", "between", "rhat", "ess")


def _map_sampler(noise):
    from ces_amd import calibrate, sample
    model, y, Gamma, mean, cov, _ = mc_.problem("elliptic", None)
    enka = calibrate.enka(2, 2, 130)
    enka.Ustar = mc_.start_ensemble("elliptic", 130, np.random.default_rng(4))
    s = sample.MCMC()
    s.mute_bar, s.y_obs, s.noise, s.trace_stride = True, y, noise, STRIDE
    prior = stats.multivariate_normal(mean=mean, cov=cov)
    return s, enka, lambda n, **kw: s.model_mh(model, n, prior, enka, Gamma, chains=M, start="ensemble", delta=0.7, **kw)


def _gp_sampler(noise):
    from ces_amd import sample
    man, a = load_gold()
    c = [c for c in man["cases"] if c["name"] == "compounded_diag"][0]
    enka = gold_problem(a, c["scaled"])
    s = sample.MCMC()
    s.mute_bar, s.y_obs, s.noise, s.trace_stride, s.seed = True, a["prob_y"], noise, STRIDE, 77
    call, prior = gold_call(a, c["kwargs"]), gold_prior(a)
    return s, enka, lambda n, **kw: s.gp_mh(enka, n, prior, chains=M, **dict(call, **kw))


def _check_marginals(m, twin_new, enka, spec_kw, n_draws, chains):
    """``m`` against numpy applied to the trace twin's states ``twin_new`` (p, 1 + kept + 1, M) after the burn-in."""
    from ces_amd import sample
    draws = cs.draws_of(twin_new, N_MCMC, STRIDE, BURN)
    p = draws.shape[1]
    assert draws.shape == (n_draws, p, chains)
    spec = sample.marginals_spec(spec_kw, enka.Ustar)
    assert m["n"] == n_draws and m["chains"] == chains
    assert np.array_equal(m["edges"], spec["edges"]) and np.array_equal(m["edges2d"], spec["edges2d"])
    assert np.array_equal(m["pairs"], spec["pairs"])
    U = np.asarray(enka.Ustar, dtype=np.float64)              # the default range is the Ustar rule
    width = 6.0 if spec_kw is True else spec_kw["width"]
    lo, hi = U.mean(axis=1) - width * U.std(axis=1, ddof=1), U.mean(axis=1) + width * U.std(axis=1, ddof=1)
    for r in range(p):
        assert np.array_equal(m["edges"][r], np.linspace(lo[r], hi[r], spec["bins"] + 1))
        assert np.array_equal(m["edges2d"][r], np.linspace(lo[r], hi[r], spec["bins2d"] + 1))
    ref = numpy_counts(draws, spec["edges"], spec["edges2d"], spec["pairs"])
    for k in COUNTS:
        assert m[k].dtype == np.int64 and np.array_equal(m[k], ref[k]), k
    check_invariants(m, n_draws, chains, spec["pairs"])
    assert np.all(m["hist1d"].sum(axis=1) > 0)                 # the range meets the posterior: the test sees real counts


def _triplets(make, fused, noise="device"):
    """The same call with summary=True alone, with marginals= as well, and with the full trace; then a resumed second call."""
    import torch
    runs = {}
    for name, kw in (("trace", {}), ("summary", dict(summary=True, burn=BURN)), ("marginals", dict(summary=True, burn=BURN, marginals=MARG))):
        s, enka, call = make(noise)
        legs = []
        for leg in range(2):
            call(N_MCMC, fused=fused, **kw)
            legs.append(dict(samples=np.array(s.samples), dev=s.samples_device.clone(), accept=s.accept, chains=np.array(s.accept_chains),
                             launches=s.fused_launches, summary=getattr(s, "summary", None), marginals=getattr(s, "marginals", None)))
        runs[name] = legs
    kept = N_MCMC // STRIDE + 2                               # the start, 13 kept states, the off-stride last
    for leg in range(2):
        a, b, c = runs["trace"][leg], runs["summary"][leg], runs["marginals"][leg]
        for other in (b, c):                                  # the chains are the same bits in all runs
            assert torch.equal(a["dev"], other["dev"]) and a["accept"] == other["accept"] and np.array_equal(a["chains"], other["chains"])
            assert a["launches"] == other["launches"] and (a["launches"] >= 1) == bool(fused)
        assert np.array_equal(b["samples"], c["samples"]) and c["samples"].shape == (a["samples"].shape[0], 2 + leg, M)
        assert a["marginals"] is None and b["marginals"] is None
        for k in SUMMARY_KEYS:                                # and so is the summary
            assert np.array_equal(b["summary"][k], c["summary"][k]), k
        first = leg * (kept - 1)                              # a resumed call counts its own draws
        _check_marginals(c["marginals"], a["samples"][:, first:, :], enka, MARG, N_DRAWS, M)
    assert not np.array_equal(runs["marginals"][0]["marginals"]["hist1d"], runs["marginals"][1]["marginals"]["hist1d"])
    s, enka, call = make(noise)                               # self.marginals is the last call's: a call without marginals= removes it
    call(N_MCMC, fused=fused, summary=True, burn=BURN, marginals=MARG)
    assert s.marginals["n"] == N_DRAWS
    call(N_MCMC, fused=fused, summary=True, burn=BURN)
    assert not hasattr(s, "marginals") and s.summary["n"] == N_DRAWS


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "steps"])
def test_model_mh_marginals_equal_numpy_on_the_trace_twin(fused):
    _triplets(_map_sampler, fused)


def test_gp_mh_marginals_equal_numpy_on_the_trace_twin():
    _triplets(_gp_sampler, False)


def test_one_chain_and_the_default_marginals():
    """M = 1 with ``marginals=True``: 64 bins, no pairs, the range 6 standard deviations of Ustar."""
    from ces_amd import calibrate, sample
    model, y, Gamma, mean, cov, _ = mc_.problem("elliptic", None)
    enka = calibrate.enka(2, 2, 130)
    enka.Ustar = mc_.start_ensemble("elliptic", 130, np.random.default_rng(4))
    prior = stats.multivariate_normal(mean=mean, cov=cov)
    out = []
    for kw in ({}, dict(summary=True, marginals=True)):
        s = sample.MCMC()
        s.mute_bar, s.y_obs, s.noise = True, y, "device"
        s.model_mh(model, 30, prior, enka, Gamma, chains=1, delta=0.7, **kw)
        out.append(s)
    plain, marg = out
    assert plain.samples.shape == (2, 31) and marg.samples.shape == (2, 2) and plain.accept == marg.accept
    assert np.array_equal(marg.samples[:, -1], plain.samples[:, -1])
    m = marg.marginals
    spec = sample.marginals_spec(True, enka.Ustar)
    assert m["n"] == 30 and m["chains"] == 1 and m["hist1d"].shape == (2, 64) and m["hist2d"].shape == (0, 20, 20)
    ref = numpy_counts(plain.samples[:, 1:].T[:, :, None], spec["edges"], spec["edges2d"], spec["pairs"])
    for k in COUNTS:
        assert np.array_equal(m[k], ref[k]), k
    # 30 draws are sparse beside a bin: the median from the counts lies within a bin width of the two order statistics that
    # numpy's median interpolates between (which may be several bins apart)
    q = sample.marginal_quantiles(m, [0.5])[:, 0]
    width = np.diff(m["edges"], axis=1)[:, 0]
    lower = np.quantile(plain.samples[:, 1:], 0.5, axis=1, method="lower")
    higher = np.quantile(plain.samples[:, 1:], 0.5, axis=1, method="higher")
    assert np.all(q >= lower - width) and np.all(q <= higher + width)
