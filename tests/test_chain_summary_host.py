"""Host conditions of the streaming chain summaries (MCMC(..., chains=M, summary=True); cesx_chain_summary_*): no GPU.

1. The numpy reference of tests/chain_summary_cases.py equals the issue's definitions written with numpy's own mean, cov and
   var at 1e-12 relative (the literal bar of tests/test_oracle_golden.py), and so does the product's finalising function fed
   the reference's raw sums.
2. Two fixed-seed sanity cases: iid chains give rhat near 1 and ess near the draw count; half the chains shifted by three
   standard deviations give a clearly larger rhat.
3. The reference made wrong on purpose -- a draw dropped, the half boundary off by one, the shift not added back, a chain left
   out, sums about zero instead of about the chain's first draw -- leaves the bounds the GPU test applies by a clear factor,
   at the shapes of the launch plan's other regimes too (``PLAN_SHAPES``: the table is held to the regimes it names from
   ``plan_of``), where three more mutants model what those regimes can get wrong: the second staged tile of every slab
   dropped, a chain of the next slab counted in a slab's ragged tile, an off-diagonal super tile formed without centring.
4. The ABI: the three entry points, the version, the new translation unit, the stage struct on the host compiler alone.
5. The argument errors that need no device."""
import ctypes
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
from scipy import stats

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chain_summary_cases as cs  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("mean", "cov", "within", "between", "rhat", "ess")
# a subset of the GPU table that has every path of the reference: one chain, an odd and an even N, p past one block
HOST_SHAPES = [(1, 1, 4), (3, 2, 5), (16, 63, 9), (17, 65, 4), (33, 130, 9), (3, 130, 5)]


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(float(np.max(np.abs(b))), 1e-300))


# ---- 1. the reference against literal numpy --------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [s for s in HOST_SHAPES if s[1] > 1], ids=str)
def test_reference_equals_literal_numpy(shape):
    """Centred family: numpy's own unshifted mean / cov / var lose |x|^2 / var digits, which is the offset family's point."""
    from ces_amd import sample
    p, J, N = shape
    x = cs.make_trace(p, J, N, "centred", "float64")
    raw = cs.ref_raw(x)
    lit = cs.literal_summary(x)
    for name, got in (("reference", cs.finalise_ref(raw)), ("finalise_summary", sample.finalise_summary(raw, N, J))):
        assert got["n"] == N and got["chains"] == J
        for k in KEYS:
            assert got[k].shape == lit[k].shape and rel(got[k], lit[k]) <= 1e-12, (name, shape, k, rel(got[k], lit[k]))


def test_offset_family_is_held_by_the_shifted_sums():
    """Around 10^4 the reference's shifted sums still equal an exact-arithmetic evaluation (centre first, then numpy) at
    1e-12, while sums about zero (the mutant) are eight digits off in the variances."""
    p, J, N = 3, 65, 9
    x = cs.make_trace(p, J, N, "offset", "float64")
    fin = cs.finalise_ref(cs.ref_raw(x))
    lit = cs.literal_summary(x - 1e4)                       # (exact: the draws are 10^4 + O(1) in fp64)
    lit["mean"] = lit["mean"] + 1e4
    for k in KEYS:
        assert rel(fin[k], lit[k]) <= 1e-12, (k, rel(fin[k], lit[k]))


def test_summary_draws_counts_the_trace_states_after_the_burn_in():
    from ces_amd import sample
    for n_mcmc, stride, burn in ((40, 3, 7), (40, 3, 0), (40, 1, 39), (12, 3, 3), (12, 5, 100), (0, 1, 0), (9, 2, 8)):
        want = sum(1 for s in range(1, n_mcmc + 1) if s % stride == 0 and s > burn)
        assert sample.summary_draws(n_mcmc, stride, burn) == want, (n_mcmc, stride, burn)
    assert sample.summary_draws(40, 3, 7) == 11
    s = np.arange(2 * 15 * 4, dtype=np.float64).reshape(2, 15, 4)          # a twin's samples: start, 13 kept, the off-stride last
    d = cs.draws_of(s, 40, 3, 7)
    assert d.shape == (11, 2, 4) and np.array_equal(d[:, 0, 0], s[0, 3:14, 0])


# ---- 2. two fixed-seed sanity cases -----------------------------------------------------------------------------------------

def _iid(shifted):
    rng = np.random.default_rng(20240)
    x = rng.standard_normal((1000, 1, 64))
    if shifted:
        x[:, :, 32:] += 3.0
    return cs.finalise_ref(cs.ref_raw(x))


def test_iid_chains_have_rhat_one_and_full_ess():
    """64 iid normal chains of 1000 draws (seed 20240): the reference gives rhat = 0.9999210 and ess = 64 000, the cap 2 M n
    (2 M var+ / B_m = 69 479: B_m = 0.001830 where iid half-chain means have 1 / 500).  The margin on |rhat - 1| is five
    times the distance observed, 7.9e-5."""
    s = _iid(False)
    assert s["n"] == 1000 and s["chains"] == 64
    assert abs(s["rhat"][0] - 0.9999210) < 1e-6 and abs(s["rhat"][0] - 1.0) < 4e-4
    assert s["ess"][0] == 64000.0
    assert abs(s["mean"][0] - 0.00063611) < 1e-7 and abs(s["cov"][0, 0] - 0.99307761) < 1e-7


def test_shifted_chains_have_a_large_rhat():
    """The same draws with chains 32 .. 63 moved by three standard deviations: B_m = 2.2796 (about 9 / 4 x 128 / 127),
    W = 0.99323 as before: rhat = 1.81471, more than 2000 of the iid case's distances from 1, and ess = 2 M var+ / B_m =
    183.658 of 64 000 draws."""
    s = _iid(True)
    assert abs(s["rhat"][0] - 1.81471) < 1e-4 and s["rhat"][0] - 1.0 > 2000 * 4e-4
    assert abs(s["ess"][0] - 183.658) < 1e-2 and s["ess"][0] < 0.01 * 64000
    assert abs(s["within"][0] - 0.99323332) < 1e-7 and abs(s["between"][0] - 2.27962841) < 1e-7


# ---- 3. the bounds see the mutants ----------------------------------------------------------------------------------------

PLAN_HOST_SHAPES = [s for s in cs.PLAN_SHAPES if s != (129, 5505, 4)]      # (left out for time: its reference takes seconds)


def test_plan_shapes_reach_the_regimes_they_name():
    """``PLAN_SHAPES`` against ``plan_of``: every regime the table's comment names is reached by the shape it names, and the
    older table reaches none of them."""
    assert cs.PLAN_SHAPES == ((64, 65, 5), (65, 130, 4), (129, 65, 5), (2, 1025, 5), (3, 32801, 4), (1, 65601, 4), (129, 5505, 4))
    assert (cs.SLAB, cs.WGS, cs.TC, cs.CH, cs.SLICES, cs.RL) == (2048, 1024, 32, 1024, 64, 32)
    src = open(os.path.join(ROOT, "ces_amd", "csrc", "kernels_chainsum.hip")).read()
    for name, v in (("CS_SLAB", cs.SLAB), ("CS_WGS", cs.WGS), ("CS_TC", cs.TC), ("CS_CH", cs.CH), ("CS_SLICES", cs.SLICES)):
        assert "constexpr int %s = %d;" % (name, v) in src, name
    assert "CS_RL = %d;" % cs.RL in src
    plan = {s: cs.plan_of(s[0], s[1]) for s in cs.PLAN_SHAPES}
    for s, pl in plan.items():
        assert (pl["cols"], pl["slabs"]) == cs.slab_plan(s[0], s[1]) and pl["cols"] % cs.TC == 0 and pl["cols"] <= cs.SLAB
        assert (pl["slabs"] - 1) * pl["cols"] < s[1] <= pl["slabs"] * pl["cols"] and 1 <= pl["last"] <= pl["cols"]
    for p in cs.P_SET:                                       # the older table: one super tile, one tile, one pass, one slice
        for J in cs.J_SET:
            pl = cs.plan_of(p, J)
            assert (pl["pairs"], pl["cols"], pl["ntile"], pl["slices"], pl["blocks"]) == (1, 32, 1, 1, 1) and pl["slabs"] <= 5
    # a full single super tile: the largest p with one pair (wave 3's block row is whole); one row more makes 3 pairs, two
    # super tiles more rows 6 (si = 2: the off-diagonal tiles (2, 0) and (2, 1))
    assert plan[(64, 65, 5)]["pairs"] == 1 and plan[(65, 130, 4)]["pairs"] == 3 and cs.plan_of(128, 130)["pairs"] == 3
    assert plan[(129, 65, 5)]["pairs"] == 6
    assert all(plan[s]["ntile"] == 1 and plan[s]["slabs"] <= 5 for s in cs.PLAN_SHAPES[:3])
    # a second pass of the reduce lanes, two slices, two workgroups of the half reduce
    pl = plan[(2, 1025, 5)]
    assert pl["slabs"] == 33 > cs.RL and (pl["slices"], pl["blocks"], pl["ntile"]) == (2, 2, 1)
    # two tiles a draw, a ragged last slab whose second tile holds one chain
    pl = plan[(3, 32801, 4)]
    assert (pl["cols"], pl["ntile"], pl["slabs"], pl["last"], pl["slices"], pl["blocks"]) == (64, 2, 513, 33, 33, 33)
    assert pl["last"] - cs.TC == 1
    # three tiles a draw, the slices at their cap below the workgroups of the half reduce
    pl = plan[(1, 65601, 4)]
    assert (pl["cols"], pl["ntile"], pl["slabs"], pl["slices"], pl["blocks"]) == (96, 3, 684, 64, 65)
    assert -(-65601 // 1024) == 65 > cs.SLICES
    # off-diagonal tiles and two tiles a draw together
    pl = plan[(129, 5505, 4)]
    assert (pl["pairs"], pl["cols"], pl["ntile"], pl["slabs"], pl["last"]) == (6, 64, 2, 87, 1)
    # each of the regimes' mutants changes something at one shape of the host's part of the table at least
    for name in ("tile_dropped", "chain_twice", "off_tile_uncentred"):
        assert any(cs.mutant_applies(name, s[0], s[1]) for s in PLAN_HOST_SHAPES), name
    assert not any(cs.mutant_applies("tile_dropped", p, J) or cs.mutant_applies("off_tile_uncentred", p, J)
                   for p in cs.P_SET for J in cs.J_SET)


@pytest.mark.parametrize("shape", HOST_SHAPES + PLAN_HOST_SHAPES, ids=str)
def test_the_bounds_hold_fp64_numpy_and_no_mutant(shape):
    """(a) the same sums in plain fp64 numpy stay inside the bounds; (b) every mutant leaves them by more than 100x in one
    output at least, in one of the two families at least (sums about zero: in the offset family).  A mutant of a plan regime
    is asked for at the shapes whose plan reaches that regime (``mutant_applies``: elsewhere it is the reference itself);
    test_plan_shapes_reach_the_regimes_they_name holds each to one such shape at least."""
    p, J, N = shape
    seen = {}
    for fam in cs.FAMILIES:
        for dtype in ("float64", "float32"):
            x = cs.make_trace(p, J, N, fam, dtype)
            ref = cs.ref_raw(x)
            bounds = cs.raw_bounds(ref)
            # (a) fp64 numpy, sequential over the draws as the kernel is
            n = N // 2
            sh = x[0]
            for h, part in enumerate((x[:n], x[N - n:])):
                S1 = np.zeros((p, J))
                S2 = np.zeros((p, J))
                for d in part:
                    S1 += d - sh
                    S2 += (d - sh) ** 2
                m, v = sh + S1 / n, (S2 - S1 * S1 / n) / (n - 1)
                assert np.all(np.abs(m - ref["half_mean"][h]) <= bounds["half_mean"][h]), (shape, fam, dtype)
                assert np.all(np.abs(v - ref["half_var"][h]) <= bounds["half_var"][h]), (shape, fam, dtype)
            dd = x - ref["c"][None, :, None]
            assert np.all(np.abs(dd.sum(axis=(0, 2)) - ref["s1"]) <= bounds["s1"])
            assert np.all(np.abs(np.tril(np.einsum("npj,nqj->pq", dd, dd)) - ref["cc"]) <= bounds["cc"])
            # (b)
            for name in cs.MUTANTS:
                if not cs.mutant_applies(name, p, J):
                    continue
                mut = cs.ref_raw(x, c=ref["c"], mutant=name)
                worst = 0.0
                for k, b in bounds.items():
                    with np.errstate(divide="ignore", invalid="ignore"):
                        r = np.abs(mut[k] - ref[k]) / b
                    r = r[np.isfinite(r)]
                    worst = max(worst, float(r.max()) if r.size else 0.0)
                seen[name] = max(seen.get(name, 0.0), worst)
    print("%s: mutants / bound %s" % (shape, {k: "%.3g" % v for k, v in seen.items()}))
    assert all(v > 100.0 for v in seen.values()), (shape, "mutants the bounds cannot see (ratio to the bound)", seen)
    assert set(seen) == {m for m in cs.MUTANTS if cs.mutant_applies(m, p, J)} and len(seen) >= 5 - (J == 1)


# ---- 4. the ABI -----------------------------------------------------------------------------------------------------------

NAMES = ("cesx_chain_summary_begin", "cesx_chain_summary_add", "cesx_chain_summary_read")


def test_abi_exports_version_and_sources():
    from ces_amd import build, engine
    build.build_lib()
    lib = engine.load_library()
    hdr = open(os.path.join(ROOT, "include", "cesx.h")).read()
    for name in NAMES:
        assert name in engine.EXPORTS and hasattr(lib, name) and name + "(" in hdr, name
    assert "#define CESX_ABI_VERSION %d" % engine.ABI_VERSION in hdr and engine.ABI_VERSION >= 8
    assert lib.cesx_abi_version() == engine.ABI_VERSION
    assert "kernels_chainsum.hip" in build.SOURCES
    assert "537 MB" in hdr and "134 MB" in hdr              # the stage's two sizes at the headline shape
    # no handle: CESX_EINVAL before anything is touched
    assert lib.cesx_chain_summary_begin(None, 8, None) == engine.EINVAL
    assert lib.cesx_chain_summary_add(None, None, 1, None) == engine.EINVAL
    assert lib.cesx_chain_summary_read(None, None, None, None, None, None, None, None, None) == engine.EINVAL


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
        cesx::ChainSumState cs;
        if (!cs.none()) return 1;
        if (cs.shift.ensure(64) || cs.S.ensure(256) || cs.c.ensure(8) || cs.cpart.ensure(8) || cs.tot.ensure(16)
            || cs.part.ensure(64) || cs.hpart.ensure(24) || cs.half.ensure(256)) return 2;
        cs.N = 8; cs.added = 3;
        if (cs.none() || live != 8) return 3;
        cs.drop();                                   /* the buffers sized by the engine stay, the read's scratch goes */
        if (!cs.none() || cs.added != 0 || live != 7 || !cs.S.get() || cs.half.get()) return 4;
    }
    if (live != 0) return 5;                         /* freed with the struct */
    std::puts("ok ChainSumState");
    return 0;
}
"""


def test_stage_struct_compiles_and_frees_on_the_host(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    src, exe = tmp_path / "chainsum_state.cpp", str(tmp_path / "chainsum_state")
    src.write_text(HOST_MAIN % os.path.join(ROOT, "ces_amd", "csrc", "cesx_stages.h"))
    build = subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-o", exe, str(src)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and run.stdout.strip() == "ok ChainSumState", (run.returncode, run.stdout, run.stderr)


# ---- 5. argument errors that need no device ---------------------------------------------------------------------------------

def _elliptic():
    from ces_amd import calibrate, sample, utils
    import map_cases as mc_
    enka = calibrate.enka(2, 2, 16)
    enka.Ustar = mc_.start_ensemble("elliptic", 16, np.random.default_rng(1))
    s = sample.MCMC()
    s.mute_bar, s.y_obs, s.noise = True, mc_.ELLIPTIC_Y, "device"
    prior = stats.multivariate_normal(mean=np.array([0.0, 100.0]), cov=np.diag([4.0, 30.0]))
    return s, utils.elliptic(), prior, enka, mc_.ELLIPTIC_GAMMA


def test_summary_needs_chains():
    s, model, prior, enka, Gamma = _elliptic()
    for kw in (dict(summary=True), dict(summary=True, burn=2), dict(burn=2)):
        with pytest.raises(ValueError, match="chains=M"):
            s.model_mh(model, 5, prior, enka, Gamma, **kw)
        enka.gpmodels = [object(), object()]
        with pytest.raises(ValueError, match="chains=M"):
            s.gp_mh(enka, 5, prior, **kw)
    assert not hasattr(s, "samples")


def test_burn_needs_summary_and_four_draws():
    s, model, prior, enka, Gamma = _elliptic()
    with pytest.raises(ValueError, match="burn"):
        s.model_mh(model, 40, prior, enka, Gamma, chains=8, burn=3)
    with pytest.raises(ValueError, match="burn"):
        s.model_mh(model, 40, prior, enka, Gamma, chains=8, burn=3, summary=False)
    for burn in (-1, 1.5, True):
        with pytest.raises(ValueError, match="burn must be"):
            s.model_mh(model, 40, prior, enka, Gamma, chains=8, summary=True, burn=burn)
    with pytest.raises(ValueError, match="summary must be"):
        s.model_mh(model, 40, prior, enka, Gamma, chains=8, summary="yes")
    s.trace_stride = 3
    for n_mcmc, burn in ((11, 0), (40, 31), (3, 0), (40, 1000)):          # 3, 3, 1 and 0 draws
        with pytest.raises(ValueError, match="leave %d draws" % (n_mcmc // 3 - min(burn, n_mcmc) // 3)):
            s.model_mh(model, n_mcmc, prior, enka, Gamma, chains=8, summary=True, burn=burn)
    assert not hasattr(s, "samples") and not hasattr(s, "_mh_eng")        # nothing was created, nothing launched
