"""Host conditions of the streaming marginals (MCMC(..., chains=M, summary=True, marginals=...); cesx_chain_hist_*): no GPU.

1. The ABI: the three entry points, the version, the descriptor's size, the new translation unit, the stage struct on the
   host compiler alone.
2. Every ValueError of ``marginals=`` that needs no device, and the pure function that turns the kwarg into edges and pairs.
3. ``marginal_quantiles`` against ``np.quantile`` on planted samples within one bin width; ``marginal_density`` integrates to
   the inside fraction.
4. ``plots.find_levels``: the level of each contour is the cell value at which the super-level mass crosses the target, the
   last entry is ``H.max()``, and the ``energy=`` and ``x, y`` forms are the ``H=`` form of their histograms."""
import ctypes
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
from scipy import stats

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cesx_chain_hist_begin", "cesx_chain_hist_add", "cesx_chain_hist_read")


# ---- 1. the ABI -----------------------------------------------------------------------------------------------------------

def test_abi_exports_version_and_sources():
    from ces_amd import build, engine
    build.build_lib()
    lib = engine.load_library()
    hdr = open(os.path.join(ROOT, "include", "cesx.h")).read()
    for name in NAMES:
        assert name in engine.EXPORTS and hasattr(lib, name) and name + "(" in hdr, name
    assert "#define CESX_ABI_VERSION %d" % engine.ABI_VERSION in hdr and engine.ABI_VERSION >= 9
    assert lib.cesx_abi_version() == engine.ABI_VERSION
    assert "kernels_chainhist.hip" in build.SOURCES
    assert "cesx_chain_hist_desc" in hdr and "528 KB" in hdr and "2.1 MB" in hdr      # the stage's sizes at p = 256
    # struct_bytes, bins, bins2d, n_pairs (4 x 32 bit), then three host pointers
    assert ctypes.sizeof(engine.ChainHistDesc) == 4 * 4 + 3 * 8
    # no handle: CESX_EINVAL before anything is touched
    d = engine.ChainHistDesc()
    assert lib.cesx_chain_hist_begin(None, ctypes.byref(d), None) == engine.EINVAL
    assert lib.cesx_chain_hist_add(None, None, 1, None) == engine.EINVAL
    assert lib.cesx_chain_hist_read(None, None, None, None, None, None) == engine.EINVAL


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
        cesx::ChainHistState ch;
        cesx::ChainSumState cs;                      /* the summary's stage is a struct of its own */
        if (!ch.none() || !cs.none()) return 1;
        if (ch.edges1.ensure(64) || ch.edges2.ensure(64) || ch.pairs.ensure(8) || ch.tot1.ensure(64) || ch.tot2.ensure(64)) return 2;
        ch.bins = 4; ch.bins2 = 2; ch.n_pairs = 1; ch.added = 3;
        if (ch.none() || live != 5) return 3;
        ch.drop();                                   /* every buffer is sized by the engine's shape: kept */
        if (!ch.none() || ch.added != 0 || ch.n_pairs != 0 || live != 5 || !ch.tot1.get() || !ch.tot2.get()) return 4;
    }
    if (live != 0) return 5;                         /* freed with the struct */
    std::puts("ok ChainHistState");
    return 0;
}
"""


def test_stage_struct_compiles_and_frees_on_the_host(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    src, exe = tmp_path / "chainhist_state.cpp", str(tmp_path / "chainhist_state")
    src.write_text(HOST_MAIN % os.path.join(ROOT, "ces_amd", "csrc", "cesx_stages.h"))
    build = subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-o", exe, str(src)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and run.stdout.strip() == "ok ChainHistState", (run.returncode, run.stdout, run.stderr)


# ---- 2. the kwarg ---------------------------------------------------------------------------------------------------------

def _elliptic():
    from ces_amd import calibrate, sample, utils
    import map_cases as mc_
    enka = calibrate.enka(2, 2, 16)
    enka.Ustar = mc_.start_ensemble("elliptic", 16, np.random.default_rng(1))
    s = sample.MCMC()
    s.mute_bar, s.y_obs, s.noise = True, mc_.ELLIPTIC_Y, "device"
    prior = stats.multivariate_normal(mean=np.array([0.0, 100.0]), cov=np.diag([4.0, 30.0]))
    return s, utils.elliptic(), prior, enka, mc_.ELLIPTIC_GAMMA


def test_marginals_need_chains_and_summary():
    s, model, prior, enka, Gamma = _elliptic()
    for kw in (dict(marginals=True), dict(marginals=dict(bins=8), summary=True)):
        with pytest.raises(ValueError, match="chains=M"):                 # the host paths have no device summary
            s.model_mh(model, 5, prior, enka, Gamma, **kw)
        enka.gpmodels = [object(), object()]
        with pytest.raises(ValueError, match="chains=M"):
            s.gp_mh(enka, 5, prior, **kw)
    for kw in (dict(), dict(summary=False), dict(summary=None)):
        with pytest.raises(ValueError, match="marginals=.*summary=True"):
            s.model_mh(model, 40, prior, enka, Gamma, chains=8, marginals=True, **kw)
    assert not hasattr(s, "samples") and not hasattr(s, "_mh_eng")        # nothing was created, nothing launched


@pytest.mark.parametrize("bad, match", [
    (dict(bin=8), "unknown key"), (dict(bins=8, nbins=3), "unknown key"), ("yes", "marginals must be"), (3, "marginals must be"),
    (dict(bins=1), "bins must be"), (dict(bins=257), "bins must be"), (dict(bins=8.0), "bins must be"), (dict(bins=True), "bins must be"),
    (dict(bins2d=1), "bins2d must be"), (dict(bins2d=65), "bins2d must be"),
    (dict(pairs="some"), "pairs must be"), (dict(pairs=[(0, 1, 2)]), "pairs must be"), (dict(pairs=[(0.0, 1.0)]), "pairs must be"),
    (dict(pairs=[(0, 0)]), "i != j"), (dict(pairs=[(0, 2)]), "i != j"), (dict(pairs=[(-1, 0)]), "i != j"),
    (dict(pairs=[(0, 1)] * 65), "at most 64"),
    (dict(range=[[0, 1]]), "range must have shape"), (dict(range=[[0, 1], [2, 2]]), "finite lo < hi"),
    (dict(range=[[0, 1], [0, np.inf]]), "finite lo < hi"),
    (dict(width=0.0), "width must be"), (dict(width=np.nan), "width must be"),
    (dict(range=[[0, 1], [1.0, 1.0 + 2 ** -50]]), "too narrow"),
], ids=str)
def test_marginals_kwarg_errors(bad, match):
    s, model, prior, enka, Gamma = _elliptic()
    with pytest.raises(ValueError, match=match):
        s.model_mh(model, 40, prior, enka, Gamma, chains=8, summary=True, marginals=bad)
    assert not hasattr(s, "samples") and not hasattr(s, "_mh_eng")


def test_all_pairs_and_the_spread_of_the_ensemble():
    from ces_amd import sample
    rng = np.random.default_rng(5)
    with pytest.raises(ValueError, match="pairs='all' is 66 pairs"):       # p = 12: 66 > 64
        sample.marginals_spec(dict(pairs="all"), rng.standard_normal((12, 30)))
    assert len(sample.marginals_spec(dict(pairs="all"), rng.standard_normal((11, 30)))["pairs"]) == 55
    U = rng.standard_normal((3, 30))
    U[1] = 2.5                                                             # no spread
    with pytest.raises(ValueError, match=r"row\(s\) \[1\].*range="):
        sample.marginals_spec(True, U)
    with pytest.raises(ValueError, match="range="):
        sample.marginals_spec(True, U[:, :1])                              # one member: no ddof = 1 spread
    U[1, 0] = np.nan
    with pytest.raises(ValueError, match="range="):
        sample.marginals_spec(True, U)
    spec = sample.marginals_spec(dict(range=[[0, 1], [2, 3], [4, 5]]), U)  # a given range does not look at Ustar
    assert np.array_equal(spec["edges"][:, [0, -1]], [[0, 1], [2, 3], [4, 5]])
    both = sample.marginals_spec(dict(range=[[0, 1], [2, 3], [4, 5]], width=3.0), U)       # width is not read beside range=
    assert np.array_equal(both["edges"], spec["edges"]) and np.array_equal(both["edges2d"], spec["edges2d"])


def test_spec_defaults_edges_and_pairs():
    from ces_amd import sample
    U = np.random.default_rng(6).standard_normal((4, 50)) * np.array([[1.0], [10.0], [0.1], [3.0]]) + 7.0
    assert sample.marginals_spec(None, U) is None and sample.marginals_spec(False, U) is None
    spec = sample.marginals_spec(True, U)
    assert spec["bins"] == 64 and spec["bins2d"] == 20 and spec["pairs"].shape == (0, 2) and spec["pairs"].dtype == np.int32
    assert spec["edges"].shape == (4, 65) and spec["edges2d"].shape == (4, 21) and spec["edges"].dtype == np.float64
    mean, std = U.mean(axis=1), U.std(axis=1, ddof=1)
    for r in range(4):                                                     # the Ustar rule, and np.linspace's own bits
        assert np.array_equal(spec["edges"][r], np.linspace(mean[r] - 6.0 * std[r], mean[r] + 6.0 * std[r], 65))
        assert np.array_equal(spec["edges2d"][r], np.linspace(mean[r] - 6.0 * std[r], mean[r] + 6.0 * std[r], 21))
    assert sample.marginals_spec({}, U)["edges"].tobytes() == spec["edges"].tobytes()
    spec = sample.marginals_spec(dict(bins=7, bins2d=3, width=2.0, pairs=[(3, 0), (1, 2)]), U)
    assert spec["pairs"].tolist() == [[3, 0], [1, 2]] and spec["edges"].shape == (4, 8) and spec["edges2d"].shape == (4, 4)
    assert np.array_equal(spec["edges"][2], np.linspace(mean[2] - 2.0 * std[2], mean[2] + 2.0 * std[2], 8))
    spec = sample.marginals_spec(dict(pairs="all", range=np.array([[0, 1]] * 4)), U)
    assert spec["pairs"].tolist() == [[0, 1], [0, 2], [0, 3], [1, 2], [1, 3], [2, 3]]
    assert np.array_equal(spec["edges2d"][3], np.linspace(0, 1, 21))
    assert sample.marginals_spec(dict(pairs=[]), U)["pairs"].shape == (0, 2)


# ---- 3. the helpers -------------------------------------------------------------------------------------------------------

def _planted(bins, lo, hi):
    """Three rows of planted samples and their marginals dict as numpy counts it."""
    rng = np.random.default_rng(11)
    x = np.stack([rng.standard_normal(20000), rng.gamma(2.0, 1.5, 20000) - 2.0, rng.uniform(-3.5, 3.5, 20000)])
    edges = np.stack([np.linspace(lo, hi, bins + 1)] * 3)
    hist = np.stack([np.histogram(x[r], bins=edges[r])[0] for r in range(3)]).astype(np.int64)
    m = dict(n=20000, chains=1, edges=edges, hist1d=hist, below=(x < lo).sum(axis=1), above=(x > hi).sum(axis=1))
    assert np.all(hist.sum(axis=1) + m["below"] + m["above"] == 20000)
    return x, m


@pytest.mark.parametrize("bins, lo, hi", [(64, -6.0, 12.0), (20, -2.5, 2.0), (256, -3.0, 3.0)])
def test_quantiles_are_within_one_bin_width(bins, lo, hi):
    """Linear within a bin from the cumulative counts: the sample quantile lies in the same bin, up to numpy's own
    interpolation between two neighbouring order statistics (which may straddle an edge: still one bin width)."""
    from ces_amd import sample
    x, m = _planted(bins, lo, hi)
    q = np.array([0.0, 0.001, 0.025, 0.16, 0.5, 0.84, 0.975, 0.999, 1.0])
    got = sample.marginal_quantiles(m, q)
    want = np.quantile(x, q, axis=1).T
    width = (hi - lo) / bins
    assert got.shape == (3, q.size)
    inside = (want >= lo) & (want <= hi)
    strictly = (want > lo + width) & (want < hi - width)
    assert np.all(np.isfinite(got[strictly])) and np.all(np.isnan(got[~inside]))
    ok = np.isfinite(got)
    assert ok.sum() >= 9 and np.all(np.abs(got - want)[ok] <= width * (1 + 1e-12)), np.abs(got - want)[ok].max() / width
    assert np.all(np.diff(got, axis=1)[ok[:, 1:] & ok[:, :-1]] >= 0)
    with pytest.raises(ValueError, match="q must lie"):
        sample.marginal_quantiles(m, [1.5])


def test_density_integrates_to_the_inside_fraction():
    from ces_amd import sample
    for bins, lo, hi in ((64, -6.0, 12.0), (20, -2.5, 2.0)):
        x, m = _planted(bins, lo, hi)
        for r in range(3):
            centres, dens = sample.marginal_density(m, r)
            assert centres.shape == dens.shape == (bins,)
            assert np.array_equal(centres, 0.5 * (m["edges"][r][:-1] + m["edges"][r][1:]))
            inside = m["hist1d"][r].sum() / 20000.0
            assert abs((dens * np.diff(m["edges"][r])).sum() - inside) <= 1e-14
    x, m = _planted(64, -6.0, 12.0)                                        # everything inside: numpy's density histogram
    assert np.allclose(sample.marginal_density(m, 0)[1], np.histogram(x[0], bins=m["edges"][0], density=True)[0], rtol=1e-14, atol=0)


# ---- 4. find_levels ---------------------------------------------------------------------------------------------------------

def _histograms():
    rng = np.random.default_rng(3)
    x, y = rng.standard_normal(30000), 0.5 * rng.standard_normal(30000) + 0.3
    y = y + 0.4 * x
    out = [np.histogram2d(x, y, bins=20)[0], np.histogram2d(x, y, bins=20, density=True)[0],
           np.histogram2d(x, y, bins=(40, 30))[0].astype(np.int64)]
    return x, y, out


def test_find_levels_cross_the_target_mass_at_a_cell_value():
    from ces_amd import plots
    contours = [.9999, .99, .95, .68]
    for H in _histograms()[2]:
        levels = plots.find_levels(H=H)
        assert len(levels) == 5 and levels[-1] == H.max()
        total = H.sum()
        values = np.unique(H)
        for c, lev in zip(contours, levels):
            assert H[H > lev].sum() <= c * total
            lower = values[values <= lev]                                  # the next-lower distinct cell value: lev itself
            assert lower.size and H[H >= lower[-1]].sum() > c * total
        assert levels[:4] == sorted(levels[:4])
    assert plots.find_levels(H=H, contours=[.5])[0] == plots.find_levels(H=H, contours=[.9, .5])[1]


def test_find_levels_forms_agree():
    from ces_amd import plots
    x, y, (Hc, Hd, _) = _histograms()
    assert plots.find_levels(x, y) == plots.find_levels(H=np.histogram2d(x, y, bins=20, density=True)[0])
    assert plots.find_levels(x, y) == plots.find_levels(H=Hd)
    E = -np.log(Hc + 1.0)                                                  # an energy whose exp(-E) has no zero cell but the outermost
    E[Hc == 0] = np.inf
    lev = plots.find_levels(H=np.exp(-E))
    en = plots.find_levels(energy=E)
    assert isinstance(en, np.ndarray) and np.array_equal(en, -np.log(lev)[::-1])
    with pytest.raises(ValueError):
        plots.find_levels()
    with pytest.raises(ValueError, match="same sign"):                     # the reference's bisect refuses this bracket too
        plots.find_levels(H=np.ones((4, 4)))
    import ces_amd.plots as mod
    src = open(mod.__file__).read()
    assert "import seaborn" not in src and "import pandas" not in src
