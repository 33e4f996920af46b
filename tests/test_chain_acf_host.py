"""Host conditions of the autocorrelation ESS (MCMC(..., chains=M, summary=True, autocorr=...); cesx_chain_acf_*): no GPU.

1. The ABI: the three entry points, header, library and bindings at one version, the cap, the new translation unit, the stage struct on the host compiler.
2. The estimator against a known answer: AR(1) chains, whose integrated autocorrelation time is (1 + phi) / (1 - phi).
3. The algebra of the shifted form the device sums, against the directly centred sums, in extended precision.
4. The elementwise bound the device test uses (tests/chain_acf_cases.py) rejects the reference made wrong in five ways.
5. Every ValueError of ``autocorr=`` that needs no device."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chain_acf_cases as ca  # noqa: E402
from test_chain_marginals_host import _elliptic  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cesx_chain_acf_begin", "cesx_chain_acf_add", "cesx_chain_acf_read")


# ---- 1. the ABI -----------------------------------------------------------------------------------------------------------

def test_abi_exports_version_and_sources():
    from ces_amd import build, engine, sample
    build.build_lib()
    lib = engine.load_library()
    hdr = open(os.path.join(ROOT, "include", "cesx.h")).read()
    for name in NAMES:
        assert name in engine.EXPORTS and hasattr(lib, name) and name + "(" in hdr, name
    assert "#define CESX_ABI_VERSION %d" % engine.ABI_VERSION in hdr and engine.ABI_VERSION >= 10
    assert lib.cesx_abi_version() == engine.ABI_VERSION
    assert "kernels_chainacf.hip" in build.SOURCES
    assert "#define CESX_CHAIN_ACF_LAGS_MAX %d" % ca.LAGS_MAX in hdr and sample.AUTOCORR_LAGS_MAX == ca.LAGS_MAX >= 63
    # no handle: CESX_EINVAL before anything is touched
    assert lib.cesx_chain_acf_begin(None, 10, 3, 1, None) == engine.EINVAL
    assert lib.cesx_chain_acf_add(None, None, 1, None) == engine.EINVAL
    assert lib.cesx_chain_acf_read(None, None, None, None, None, None, None) == engine.EINVAL


HOST_MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include "%s"
static int live = 0;
namespace cesx {
int dev_alloc(void** p, size_t bytes, bool zero) { *p = zero ? calloc(1, bytes ? bytes : 8) : malloc(bytes ? bytes : 8); ++live; return 0; }
void dev_free(void* p) { free(p); --live; }
}
int main() {
    {
        cesx::ChainAcfState ca;
        cesx::ChainSumState cs;                      /* the summary's stage is a struct of its own */
        if (!ca.none() || !cs.none()) return 1;
        if (ca.c.ensure(64) || ca.S1.ensure(64) || ca.P.ensure(64) || ca.ring.ensure(64) || ca.head.ensure(64) || ca.pending.ensure(64)
            || ca.out.ensure(64) || ca.gamma.ensure(64) || ca.mean.ensure(64)) return 2;
        ca.N = 9; ca.added = 3; ca.done = 0; ca.pend = 3; ca.L = 2; ca.LT = 8; ca.C = 1;
        if (ca.none() || live != 9) return 3;
        ca.drop();                                   /* the run's buffers are kept for the next begin; a read's outputs go */
        if (!ca.none() || ca.added != 0 || ca.pend != 0 || live != 7 || !ca.P.get() || ca.gamma.get()) return 4;
    }
    if (live != 0) return 5;                         /* freed with the struct */
    std::puts("ok ChainAcfState");
    return 0;
}
"""


def test_stage_struct_compiles_and_frees_on_the_host(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    src, exe = tmp_path / "chainacf_state.cpp", str(tmp_path / "chainacf_state")
    src.write_text(HOST_MAIN % os.path.join(ROOT, "ces_amd", "csrc", "cesx_stages.h"))
    build = subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-o", exe, str(src)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and run.stdout.strip() == "ok ChainAcfState", (run.returncode, run.stdout, run.stderr)


# ---- 2. the estimator against a known answer ----------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ar1_runs():
    """The issue's three AR(1) runs, each from ``np.random.default_rng(7)``: (phi, n, M, L) -> (p, n, M) draws."""
    return {(phi, n, M, L): ca.ar1(phi, 3, n, M, np.random.default_rng(7))
            for phi, n, M, L in ((0.5, 2000, 64, 31), (0.95, 2000, 64, 31), (0.0, 500, 8, 7))}


def test_ar1_half_is_within_ten_percent(ar1_runs):
    from ces_amd import sample
    phi, n, M, L = 0.5, 2000, 64, 31
    out = sample.autocorr_of_samples(ar1_runs[(phi, n, M, L)], L)
    eff = out["ess"] / (M * n)
    print("\n[chain acf] AR(1) phi = 0.5: ESS / (M n) = %s against %.4f" % (np.round(eff, 4), (1 - phi) / (1 + phi)))
    assert out["n"] == n and out["chains"] == M and out["lags"] == L and out["rho"].shape == (3, L + 1)
    assert not out["truncated"].any()
    assert np.all(np.abs(eff / ((1 - phi) / (1 + phi)) - 1) <= 0.10), eff
    assert np.all(out["rho"][:, 0] == 1.0) and np.all(np.abs(out["rho"][:, 1] - phi) < 0.02)
    assert np.all(np.abs(out["var_plus"] / (1 / (1 - phi * phi)) - 1) < 0.05)


def test_ar1_slow_chain_is_flagged_truncated(ar1_runs):
    from ces_amd import sample
    phi, n, M, L = 0.95, 2000, 64, 31
    out = sample.autocorr_of_samples(ar1_runs[(phi, n, M, L)], L)
    eff = out["ess"] / (M * n)
    print("\n[chain acf] AR(1) phi = 0.95, L = 31: ESS / (M n) = %s against %.4f, truncated %s"
          % (np.round(eff, 4), (1 - phi) / (1 + phi), out["truncated"]))
    assert out["truncated"].all()
    assert np.all(eff > (1 - phi) / (1 + phi))             # the flag's meaning: an over-estimate


def test_white_noise_is_within_ten_percent_of_one(ar1_runs):
    from ces_amd import sample
    phi, n, M, L = 0.0, 500, 8, 7
    out = sample.autocorr_of_samples(ar1_runs[(phi, n, M, L)], L)
    eff = out["ess"] / (M * n)
    print("\n[chain acf] white noise: ESS / (M n) = %s" % np.round(eff, 4))
    assert np.all(np.abs(eff - 1) <= 0.10), eff


def test_finalise_is_the_definition_written_out():
    """``finalise_autocorr`` on the raw sums of a trace against ``estimator_ref``, and ``M_total`` scaling the ESS alone."""
    from ces_amd import sample
    x = ca.ar1(0.8, 4, 300, 6, np.random.default_rng(3)) + 50.0
    for L in (1, 2, 9, 31):
        raw = sample.autocorr_raw_of_samples(x, L)
        out = sample.finalise_autocorr(raw, 300, 24, 6, L)
        rho, tau, ess, trunc, W, vp = ca.estimator_ref(raw, 300, 24, 6, L)
        for got, want in ((out["rho"], rho), (out["tau"], tau), (out["ess"], ess), (out["within"], W), (out["var_plus"], vp)):
            assert np.allclose(got, want, rtol=1e-12, atol=0, equal_nan=True)
        assert np.array_equal(out["truncated"], trunc)
        assert np.allclose(out["ess"] * 6 / 24, sample.finalise_autocorr(raw, 300, 6, 6, L)["ess"], rtol=1e-15)
    one = sample.autocorr_of_samples(x[:, :, 0], 9)         # (p, n): one chain, B = 0
    assert one["chains"] == 1 and np.allclose(one["var_plus"], 299 / 300 * one["within"], rtol=1e-14)


# ---- 3. the algebra ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("L,N", [(1, 4), (5, 7), (31, 33), (31, 40), (31, 61), (64, 66), (64, 100), (7, 200)],
                         ids=lambda v: str(v))
def test_shifted_form_is_the_centred_sum(L, N):
    """N = L + 2, overlapping head and tail windows (N < 2 L) and long chains: the device's form about the first draw equals
    sum (x_t - m)(x_{t+k} - m) to a few roundings of the extended precision both are computed in."""
    x = ca.make_trace(3, 5, N, "float64", seed=L)
    a, b = ca.ref_raw(x, 5, L, form="shifted"), ca.ref_raw(x, 5, L)
    tol = 64 * N * float(np.finfo(np.longdouble).eps) * a["B_chain_gamma"] + 2 * 2.0 ** -53 * np.abs(b["chain_gamma"])
    assert np.all(np.abs(a["chain_gamma"] - b["chain_gamma"]) <= tol)
    assert np.all(a["chain_gamma"][:, :, 2] == 0) and np.all(b["chain_gamma"][:, :, 2] == 0)       # the stuck chain


def test_constant_chains_give_nan_only_when_all_are_constant():
    from ces_amd import sample
    x = ca.ar1(0.3, 2, 40, 3, np.random.default_rng(1))
    x[0, :, 1] = 0.0                                        # one constant chain in row 0: the others carry the row
    out = sample.autocorr_of_samples(x, 5)
    assert np.all(np.isfinite(out["ess"])) and np.all(np.isfinite(out["rho"]))
    x[0] = 0.0                                              # every chain of row 0 constant (all zeros)
    with np.errstate(all="raise"):                          # and no warning storm
        out = sample.autocorr_of_samples(x, 5)
    assert np.isnan(out["ess"][0]) and np.isnan(out["tau"][0]) and not out["truncated"][0] and out["var_plus"][0] == 0
    assert np.isfinite(out["ess"][1])
    raw = sample.autocorr_raw_of_samples(x, 5)
    assert np.all(raw["chain_gamma"][:, 0, :] == 0) and np.all(raw["gsum"][0] == 0)


# ---- 4. the bound has teeth ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mutant", ca.MUTANTS)
@pytest.mark.parametrize("L,N", [(2, 11), (31, 98)], ids=lambda v: str(v))
def test_the_bound_rejects_the_mutants(mutant, L, N):
    """Each mutant leaves the bound of ``raw_bounds`` in chain_gamma and in gsum: on the ordinary chain 0 and -- sums about
    zero -- on chain 1, whose mean is 10^6 x its spread."""
    p, J, C = 3, 5, 4
    x = ca.make_trace(p, J, N, "float64", seed=11)
    ref = ca.ref_raw(x, C, L)
    bounds = ca.raw_bounds(ref)
    bad = ca.ref_raw(x, C, L, mutant=mutant, boundary=max(1, N // 2))
    chain = 1 if mutant == "sums_about_zero" else 0
    err = np.abs(bad["chain_gamma"] - ref["chain_gamma"])[:, :, chain]
    bnd = bounds["chain_gamma"][:, :, chain]
    rows = slice(1, None) if mutant in ("lag_off_by_one", "history_not_carried", "no_head_tail") else slice(None)   # lag 0 has neither
    assert np.all(err[rows] > bnd[rows]), (mutant, float(np.min(err[rows] / bnd[rows])))
    assert np.any(np.abs(bad["gsum"] - ref["gsum"]) > bounds["gsum"]), mutant
    same = ca.ref_raw(x, C, L, form="shifted")                # (and the bound passes the device's own form)
    assert np.all(np.abs(same["chain_gamma"] - ref["chain_gamma"]) <= 1e-3 * bounds["chain_gamma"])


# ---- 5. the kwarg -----------------------------------------------------------------------------------------------------------------

def test_autocorr_needs_chains_and_summary():
    s, model, prior, enka, Gamma = _elliptic()
    for kw in (dict(autocorr=True), dict(autocorr=dict(lags=3), summary=True)):
        with pytest.raises(ValueError, match="chains=M"):                 # the host paths have no device summary
            s.model_mh(model, 5, prior, enka, Gamma, **kw)
        enka.gpmodels = [object(), object()]
        with pytest.raises(ValueError, match="chains=M"):
            s.gp_mh(enka, 5, prior, **kw)
    for kw in (dict(), dict(summary=False), dict(summary=None)):
        with pytest.raises(ValueError, match="autocorr=.*summary=True"):
            s.model_mh(model, 40, prior, enka, Gamma, chains=8, autocorr=True, **kw)
    assert not hasattr(s, "samples") and not hasattr(s, "_mh_eng")        # nothing was created, nothing launched


@pytest.mark.parametrize("bad, match", [
    (dict(lag=8), "unknown key"), (dict(lags=8, chain=3), "unknown key"), ("yes", "autocorr must be"), (3.0, "autocorr must be"),
    (dict(lags=0), "lags must be"), (0, "lags must be"), (-1, "lags must be"), (dict(lags=65), "lags must be"), (65, "lags must be"),
    (dict(lags=8.0), "lags must be"), (dict(lags=True), "lags must be"),
    (dict(chains=0), "chains must be"), (dict(chains=9), "chains must be"), (dict(chains=2.0), "chains must be"),
    (39, "fewer than lags \\+ 2"), (dict(lags=40, chains=2), "fewer than lags \\+ 2"),
], ids=str)
def test_autocorr_kwarg_errors(bad, match):
    s, model, prior, enka, Gamma = _elliptic()
    with pytest.raises(ValueError, match=match):
        s.model_mh(model, 40, prior, enka, Gamma, chains=8, summary=True, autocorr=bad)
    assert not hasattr(s, "samples") and not hasattr(s, "_mh_eng")


def test_spec_defaults():
    from ces_amd import sample
    assert sample.autocorr_spec(None, 8, True, 40) is None and sample.autocorr_spec(False, 8, False, 0) is None
    assert sample.autocorr_spec(True, 8, True, 40) == (31, 8)
    assert sample.autocorr_spec(True, 65536, True, 40) == (31, 1024)
    assert sample.autocorr_spec(7, 65536, True, 9) == (7, 1024)
    assert sample.autocorr_spec(dict(lags=64, chains=65536), 65536, True, 66) == (64, 65536)
    with pytest.raises(ValueError, match="fewer than lags"):
        sample.autocorr_spec(dict(lags=64), 8, True, 65)
    with pytest.raises(ValueError, match="fewer than lags"):               # the stage's own minimum of 4 draws
        sample.autocorr_spec(1, 8, True, 3)
