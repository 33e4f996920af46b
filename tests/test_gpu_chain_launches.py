"""The Python chain driver across fused launches (MCMC._mh_device: model_mh / gp_mh with chains=M, fused=True).

A fused run is cut into the launches of ``sample.fused_chunks``; at the product's caps (4096 steps, 64 MiB, GP_FUSED_WORK)
only a long production run has more than one.  Here the caps are lowered on the sampler instance -- ``FUSED_STEPS_MAX`` = 40,
9 or 2, for gp_mh ``GP_FUSED_WORK`` = 9 or 2 steps' work -- so that 40- and 38-step runs at trace_stride 3 make several:

    cap 9   K_max = 9: launches of 9, 9, 9, 9 and 4 (or 2) steps; the last one keeps one state (or none)
    cap 2   K_max = the stride, 3: thirteen (twelve) launches of one kept state and a last one of 1 (2) steps that keeps none
            (K // stride == 0: no trace pointer)
    cap 40  K_max = 39: 38 steps are one launch, 40 steps are 39 + 1
    none    the product's caps: one launch, the control

1. fp64 engine, device noise: phi and the states cross a launch in fp64, so every multi-launch run is the single launch bit
   for bit -- ``samples``, ``samples_device``, ``accept_chains``, ``accept``, ``_mh_next_step`` -- and so is a resumed second
   call.  ``fused_launches`` is the count written out below.
2. The same with ``noise='numpy'`` under one seed: the draws are stacked per launch in the step loop's order, and numpy's
   global generator ends where the step path leaves it.
3. fp32 engine: the states are rounded where a launch ends, so a multi-launch run is not the single launch; the trace twin
   and the ``summary=True`` twin under the same caps are the same chains bit for bit.
4. ``summary=True, burn=b`` with ``marginals=`` under caps 9 and 2, b = 7, 13, 18 -- inside the first launch, inside the second
   (its first kept state left out), exactly two launches (the second skipped whole): 11, 9 and 7 draws.  The chains are the
   trace twin's bits, ``summary`` is the reference on the twin's draws under ``cs.summary_bounds``, the counts are numpy's on
   those draws, ``samples`` holds the start state and the last state, a resumed call summarises its own draws.

Measured on an MI355X: NOTEBOOK.md, "Streaming chain summaries"."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chain_summary_cases as cs  # noqa: E402
import gp_chain_cases as gc  # noqa: E402
import map_cases as mc_  # noqa: E402
from test_gpu_chain_marginals import COUNTS, check_invariants, numpy_counts  # noqa: E402
from test_gpu_chain_summary import M, STRIDE, _gp_sampler, _map_sampler  # noqa: E402

gpu = pytest.mark.gpu                                         # every test but the table's own check, which needs no device
M_GP = 65
# (n_mcmc, cap) -> the launches of the run, written out (cap None: the product's caps)
CHUNKS = {(40, None): [40], (38, None): [38], (40, 40): [39, 1], (38, 40): [38],
          (40, 9): [9, 9, 9, 9, 4], (38, 9): [9, 9, 9, 9, 2], (40, 2): [3] * 13 + [1], (38, 2): [3] * 12 + [2]}
LAUNCHES = {(40, None): 1, (38, None): 1, (40, 40): 2, (38, 40): 1, (40, 9): 5, (38, 9): 5, (40, 2): 14, (38, 2): 13}
KEPT = {40: 15, 38: 14}                                       # the start, n // 3 kept states, the off-stride last


def test_the_launch_table_is_fused_chunks():
    """The literal table against the pure function the driver calls (no device work: it is here beside its table)."""
    from ces_amd import sample
    assert STRIDE == 3 and M == 130
    for (n, cap), chunks in CHUNKS.items():
        K_max, got = sample.fused_chunks(n, STRIDE, sample.MCMC.FUSED_STEPS_MAX if cap is None else cap, 64 << 20, 1)
        assert got == chunks and len(chunks) == LAUNCHES[(n, cap)] and sum(chunks) == n and K_max % STRIDE == 0, (n, cap)
        K_max, got = sample.fused_chunks(n, STRIDE, 4096, 64 << 20, 1, None if cap is None else cap * 1000, 1000)
        assert got == chunks, (n, cap, "the work cap")
    assert CHUNKS[(40, 2)][-1] // STRIDE == 0 and CHUNKS[(38, 2)][-1] // STRIDE == 0      # a last launch that keeps no state


# ---- the samplers and their caps ---------------------------------------------------------------------------------------------

def _map_make(kind, update=None):
    def make(noise):
        s, call = _map_sampler(kind, noise)
        if update is None:
            return s, call
        return s, lambda n, **kw: call(n, update=update, beta=mc_.BETA[kind], **kw)
    return make


def _gp_case(mode):
    """One case of tests/gp_chain_cases.py per likelihood mode, at M = 65 (three tiles of chains, the last of one)."""
    i = {"gamma": 7, "var": 2, "gamma_var": 9, "gamma_dense": 4}[mode]
    c = dict(gc.cases()[i], M=M_GP)
    assert c["mode"] == mode
    return c


def _gp_make(c):
    def make(noise):
        from ces_amd import sample
        enka, y, prior, kw = gc.problem(c)
        s = sample.MCMC()
        s.mute_bar, s.y_obs, s.noise, s.seed, s.trace_stride = True, y, noise, gc.SEED, STRIDE
        return s, lambda n, **k: s.gp_mh(enka, n, prior, chains=c["M"], **dict(kw, **k))
    return make


def _gp_work(c):
    """The arithmetic of one fused step of all chains, in the unit of ``GP_FUSED_WORK``: M n_gp J_p (J_p // 2 + p + 8)."""
    from ces_amd import emulate
    enka = gc.problem(c)[0]
    Jp = (int(emulate.device_image(enka, enka.gpmodels)["Jt"]) + 15) // 16 * 16
    assert Jp == (c["Jt"] + 15) // 16 * 16
    return c["M"] * enka.n_obs * Jp * (Jp // 2 + enka.p + 8)


def _steps_cap(cap):
    def set_cap(s):
        if cap is not None:
            s.FUSED_STEPS_MAX = cap
    return set_cap


def _work_cap(cap, work):
    def set_cap(s):
        if cap is not None:
            s.GP_FUSED_WORK = cap * work
    return set_cap


def _legs(make, n_mcmc, set_cap, noise="device", seed=None, dtype=None, fused=True, **kw):
    """A fresh call and a resumed second one of a new sampler with the caps ``set_cap`` puts on the instance."""
    from ces_amd import sample
    s, call = make(noise)
    set_cap(s)
    if dtype is not None:
        s.engine_dtype = dtype
    legs = []
    for leg in range(2):
        if seed is not None:
            np.random.seed(seed + leg)
        call(n_mcmc, fused=fused, **kw)
        legs.append(dict(samples=np.array(s.samples), dev=s.samples_device.cpu().numpy().copy(), accept=s.accept,
                         chains=np.array(s.accept_chains), launches=s.fused_launches, next=s._mh_next_step,
                         summary=getattr(s, "summary", None), marginals=getattr(s, "marginals", None),
                         rng=np.random.get_state() if seed is not None else None))
    assert (sample.MCMC.FUSED_STEPS_MAX, sample.MCMC.FUSED_BUFFER_BYTES) == (4096, 64 << 20)      # the product is as it was
    assert sample.MCMC.GP_FUSED_WORK == 50 * 65536 * 32 * 512 * (512 // 2 + 8 + 8)
    return legs


def _same_rng(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def _assert_same_run(a, b, tag):
    for leg in range(2):
        for k in ("samples", "dev", "chains"):
            assert a[leg][k].shape == b[leg][k].shape and np.array_equal(a[leg][k], b[leg][k]), (tag, leg, k)
        assert a[leg]["accept"] == b[leg]["accept"] and a[leg]["next"] == b[leg]["next"], (tag, leg)


def _assert_a_real_run(legs, n_mcmc, chains, tag):
    """The control moves: proposals are accepted and rejected alike, and the shapes are the trace's."""
    p = legs[0]["samples"].shape[0]
    for leg in range(2):
        a = legs[leg]
        assert a["samples"].shape == (p, KEPT[n_mcmc] + leg * (KEPT[n_mcmc] - 1), chains), tag
        assert a["next"] == n_mcmc * (leg + 1) and 0.0 < a["accept"] < 1.0, (tag, a["accept"])
        assert np.array_equal(a["samples"][:, -1, :], a["dev"]) and np.all(np.isfinite(a["samples"])), tag
    assert not np.array_equal(legs[0]["dev"], legs[1]["dev"]) and not np.array_equal(legs[0]["samples"][:, 0, :], legs[0]["dev"])


def _across_launches(make, caps, chains, noise="device", seed=None):
    """Conditions 1 and 2: every capped run against the single launch, fresh and resumed, at 40 and 38 steps."""
    for n_mcmc in (40, 38):
        control = _legs(make, n_mcmc, caps[None], noise, seed)
        _assert_a_real_run(control, n_mcmc, chains, n_mcmc)
        assert [leg["launches"] for leg in control] == [1, 1]
        steps = _legs(make, n_mcmc, caps[None], noise, seed, fused=False) if seed is not None else None
        for cap, set_cap in caps.items():
            if cap is None:
                continue
            run = _legs(make, n_mcmc, set_cap, noise, seed)
            _assert_same_run(run, control, (n_mcmc, cap))
            assert [leg["launches"] for leg in run] == [LAUNCHES[(n_mcmc, cap)]] * 2, (n_mcmc, cap)
            if seed is not None:                              # numpy's generator ends where the step path leaves it
                for leg in range(2):
                    assert _same_rng(run[leg]["rng"], steps[leg]["rng"]) and _same_rng(control[leg]["rng"], steps[leg]["rng"])
                    assert steps[leg]["launches"] == 0


STEP_CAPS = {None: _steps_cap(None), 40: _steps_cap(40), 9: _steps_cap(9), 2: _steps_cap(2)}


def _gp_caps(c):
    work = _gp_work(c)
    return {None: _steps_cap(None), 40: _steps_cap(40), 9: _work_cap(9, work), 2: _work_cap(2, work)}


# ---- 1. fp64, device noise ---------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("update", [None, "pCN"], ids=["rw", "pcn"])
@pytest.mark.parametrize("kind", ["banana", "elliptic"])
def test_model_mh_across_launches_is_the_single_launch(kind, update):
    _across_launches(_map_make(kind, update), STEP_CAPS, M)


@gpu
@pytest.mark.parametrize("mode", ["gamma", "var", "gamma_var", "gamma_dense"])
def test_gp_mh_across_launches_is_the_single_launch(mode):
    """The launches 9 and 2 steps long come from ``GP_FUSED_WORK`` alone: ``FUSED_STEPS_MAX`` stays 4096 there."""
    c = _gp_case(mode)
    _across_launches(_gp_make(c), _gp_caps(c), M_GP)


# ---- 2. injected noise -------------------------------------------------------------------------------------------------------

@gpu
def test_model_mh_across_launches_with_numpy_noise():
    _across_launches(_map_make("banana"), STEP_CAPS, M, noise="numpy", seed=31)


@gpu
def test_gp_mh_across_launches_with_numpy_noise():
    c = _gp_case("gamma_var")
    _across_launches(_gp_make(c), _gp_caps(c), M_GP, noise="numpy", seed=47)


# ---- 3. the fp32 engine --------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("which", ["model_mh", "gp_mh"])
def test_fp32_twins_are_the_same_chains_across_launches(which):
    make = _map_make("banana") if which == "model_mh" else _gp_make(_gp_case("gamma"))
    caps = STEP_CAPS if which == "model_mh" else _gp_caps(_gp_case("gamma"))
    chains = M if which == "model_mh" else M_GP
    for cap in (9, 2):
        plain = _legs(make, 40, caps[cap], dtype="float32")
        summed = _legs(make, 40, caps[cap], dtype="float32", summary=True, burn=7)
        _assert_a_real_run(plain, 40, chains, (which, cap))
        p = plain[0]["samples"].shape[0]
        for leg in range(2):
            a, b = plain[leg], summed[leg]
            assert a["launches"] == b["launches"] == LAUNCHES[(40, cap)]
            assert np.array_equal(a["dev"], b["dev"]) and np.array_equal(a["chains"], b["chains"]), (which, cap, leg)
            assert a["accept"] == b["accept"] and a["next"] == b["next"]
            assert b["samples"].shape == (p, 2 + leg, chains)
            assert np.array_equal(b["samples"][:, -1, :], a["samples"][:, -1, :])
            assert np.array_equal(b["samples"][:, 0, :], a["samples"][:, 0, :])
            assert b["summary"]["n"] == 11 and a["summary"] is None and a["dev"].dtype == np.float32


# ---- 4. summaries and marginals across launches --------------------------------------------------------------------------------

BURNS = {7: 11, 13: 9, 18: 7}                                 # burn -> draws of a 40-step call at stride 3
SUMMARY_KEYS = ("mean", "cov", "within", "between", "rhat", "ess")


def _check_summary(summary, twin_new, burn, p, chains, tag):
    draws = cs.draws_of(twin_new, 40, STRIDE, burn)
    assert draws.shape == (BURNS[burn], p, chains), tag
    ref = cs.ref_raw(draws)
    want, bounds = cs.finalise_ref(ref), cs.summary_bounds(ref)
    assert summary["n"] == BURNS[burn] and summary["chains"] == chains
    for k, b in bounds.items():
        assert summary[k].shape == want[k].shape and summary[k].dtype == np.float64
        assert np.all(np.abs(summary[k] - want[k]) <= b), (tag, k, float(np.max(np.abs(summary[k] - want[k]) / b)))
    return draws


@gpu
@pytest.mark.parametrize("cap", [9, 2])
@pytest.mark.parametrize("which", ["model_mh", "gp_mh"])
def test_summary_and_marginals_across_launches(which, cap):
    make = _map_make("banana") if which == "model_mh" else _gp_sampler
    twin = _legs(make, 40, _steps_cap(cap))
    _assert_a_real_run(twin, 40, M, (which, cap))
    p = twin[0]["samples"].shape[0]
    # a range that cuts the chains' own spread: below and above are counted too
    lo, hi = (np.quantile(twin[0]["samples"], q, axis=(1, 2)) for q in (0.05, 0.9))
    marg = dict(bins=24, bins2d=20, pairs=[(0, 1), (1, 0)], range=np.stack([lo, hi], axis=1))
    alone = _legs(make, 40, _steps_cap(cap), summary=True, burn=13)
    for burn, n_draws in BURNS.items():
        run = _legs(make, 40, _steps_cap(cap), summary=True, burn=burn, marginals=marg)
        for leg in range(2):
            a, b = twin[leg], run[leg]
            tag = (which, cap, burn, leg)
            assert a["launches"] == b["launches"] == LAUNCHES[(40, cap)], tag
            assert np.array_equal(a["dev"], b["dev"]) and np.array_equal(a["chains"], b["chains"]), tag
            assert a["accept"] == b["accept"] and a["next"] == b["next"] == 40 * (leg + 1), tag
            assert b["samples"].shape == (p, 2 + leg, M), tag                        # the start state, the calls' last states
            assert np.array_equal(b["samples"][:, 0, :], a["samples"][:, 0, :]), tag
            assert np.array_equal(b["samples"][:, -1, :], a["samples"][:, -1, :]), tag
            first = leg * (KEPT[40] - 1)                      # a resumed call summarises its own draws
            draws = _check_summary(b["summary"], a["samples"][:, first:, :], burn, p, M, tag)
            m = b["marginals"]
            assert m["n"] == n_draws and m["chains"] == M
            for r in range(p):
                assert np.array_equal(m["edges"][r], np.linspace(lo[r], hi[r], 25)), tag
                assert np.array_equal(m["edges2d"][r], np.linspace(lo[r], hi[r], 21)), tag
            ref = numpy_counts(draws, m["edges"], m["edges2d"], m["pairs"])
            for k in COUNTS:
                assert m[k].dtype == np.int64 and np.array_equal(m[k], ref[k]), (tag, k)
            check_invariants(m, n_draws, M, m["pairs"])
            assert np.all(m["hist1d"].sum(axis=1) > 0) and (m["below"] + m["above"]).sum() > 0, tag
            if burn == 13:                                    # summary=True alone: the same summary bits
                for k in SUMMARY_KEYS:
                    assert np.array_equal(alone[leg]["summary"][k], b["summary"][k]), (tag, k)
                assert alone[leg]["marginals"] is None and np.array_equal(alone[leg]["samples"], b["samples"])
        assert not np.array_equal(run[0]["summary"]["mean"], run[1]["summary"]["mean"])
