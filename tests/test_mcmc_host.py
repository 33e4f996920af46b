"""The Sample stage's drop-in MCMC class on the host (ces_amd/sample.py) against chains of the real reference's
ces/sample.py (tests/golden/mcmc.npz, written by tools/make_golden_mcmc.py), its interface, and the C ABI of the
device path (declared, exported, no scratch)."""
import inspect
import json
import os
import re
import sys

import numpy as np
import pytest
from scipy import stats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
MH_ENTRY_POINTS = ("cesx_mh_set_proposal", "cesx_mh_start", "cesx_mh_propose", "cesx_mh_accept", "cesx_mh_stats")


def load_cases():
    with open(os.path.join(GOLD, "mcmc_manifest.json")) as fh:
        cases = json.load(fh)
    arrays = np.load(os.path.join(GOLD, "mcmc.npz"))
    out = []
    for c in cases:
        tag = c["name"] + "_"
        out.append((c, {k[len(tag):]: arrays[k] for k in arrays.files if k.startswith(tag)}))
    return out


def setup_case(c, a):
    """The reference run's objects, rebuilt with this package's classes."""
    from ces_amd import calibrate, sample, utils
    model = utils.lineal(a["A"])
    enka = calibrate.enka(c["p"], c["n_obs"], c["J"])
    enka.Ustar = a["Ustar"]
    prior = stats.multivariate_normal(mean=a["mu"], cov=a["Sigma"])
    mc = sample.MCMC()
    mc.mute_bar = True
    mc.y_obs = a["y"]
    return mc, model, enka, prior


def run_case(c, a, **extra):
    mc, model, enka, prior = setup_case(c, a)
    kw = dict(c["kwargs"], **extra)
    np.random.seed(c["seed"])
    if c["resume"]:
        mc.model_mh(model, c["resume"], prior, enka, a["Gamma"], **kw)
        mc.model_mh(model, c["steps"] - c["resume"], prior, enka, a["Gamma"], **kw)
    else:
        mc.model_mh(model, c["steps"], prior, enka, a["Gamma"], **kw)
    return mc


@pytest.mark.parametrize("case", [c["name"] for c, _ in load_cases()])
def test_host_model_mh_matches_reference(case):
    c, a = next((c, a) for c, a in load_cases() if c["name"] == case)
    mc = run_case(c, a)
    assert mc.samples.shape == a["samples"].shape
    np.testing.assert_allclose(mc.samples, a["samples"], rtol=1e-12, atol=1e-12)
    assert abs(mc.accept - float(a["accept"])) < 1e-12


def test_reference_interface():
    from ces_amd import sample
    mc = sample.MCMC()
    assert mc.mute_bar is False
    sig = inspect.signature(sample.MCMC.model_mh)
    assert list(sig.parameters)[:8] == ["self", "model", "n_mcmc", "prior", "enka", "Gamma", "delta", "enka_scaling"]
    assert sig.parameters["delta"].default == 1. and sig.parameters["enka_scaling"].default is True
    assert "kwargs" in sig.parameters
    sig = inspect.signature(sample.MCMC.gp_mh)
    assert list(sig.parameters)[:6] == ["self", "enka", "n_mcmc", "prior", "delta", "enka_scaling"]
    assert list(inspect.signature(sample.MCMC.random_walk).parameters) == ["self", "current", "scales", "n_dim"]
    sig = inspect.signature(sample.MCMC.pCN)
    assert list(sig.parameters) == ["self", "current", "scales", "n_dim", "beta"] and sig.parameters["beta"].default == 0.5
    # nothing of the Calibrate module is re-exported
    assert not hasattr(sample, "sampling") and not hasattr(sample, "enka")


def test_pcn_step_uses_sqrt_beta():
    from ces_amd import sample
    mc = sample.MCMC()
    S = np.array([[2.0, 0.0], [0.5, 1.0]])
    u = np.array([1.0, -1.0])
    np.random.seed(3)
    got = mc.pCN(u, S, 2, beta=0.3)
    np.random.seed(3)
    xi = np.random.normal(0, 1, 2)
    assert np.allclose(got, np.sqrt(1 - 0.09) * u + np.sqrt(0.3) * S @ xi, rtol=1e-15)


def test_gp_mh_raises_import_error():
    from ces_amd import sample
    with pytest.raises(ImportError, match="GPflow"):
        sample.MCMC().gp_mh(None, 10, None)


def test_chains_rejects_models_without_a_device_map():
    from ces_amd import calibrate, models, sample
    mc = sample.MCMC()
    mc.y_obs = np.zeros(9)
    enka = calibrate.enka(2, 9, 8)
    enka.Ustar = np.random.default_rng(0).standard_normal((2, 8))
    prior = stats.multivariate_normal(mean=np.zeros(2), cov=np.eye(2))
    with pytest.raises(ValueError, match="forward_device"):
        mc.model_mh(models.lorenz63(l_window=2, freq=25), 5, prior, enka, np.eye(9), chains=4)

    class HostMap:                   # a 'map' model without the device hook
        type = "map"

        def __call__(self, theta):
            return np.zeros(9)
    with pytest.raises(ValueError, match="forward_device"):
        mc.model_mh(HostMap(), 5, prior, enka, np.eye(9), chains=1)


def _declared():
    text = open(os.path.join(ROOT, "include", "cesx.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(cesx_[a-z_]+)\s*\(", text))


def test_mh_entry_points_declared_and_exported():
    from ces_amd import build, engine
    names = _declared()
    for name in MH_ENTRY_POINTS:
        assert name in names, name
        assert name in engine.EXPORTS, name
    lib = engine.load_library(build.build_lib())
    for name in MH_ENTRY_POINTS:
        assert hasattr(lib, name), name


def test_mh_kernels_have_no_scratch_and_no_spills():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_audit
    t = isa_audit.collect(["kernels_mh.hip"])
    rows = {k: v for k, v in t.items() if "mh_accept_kernel" in k}
    assert len(rows) == 4                               # {float, double} x {16-byte, scalar loads}
    for name, r in rows.items():
        assert r["ScratchSize [bytes/lane]"] == 0, name
        assert r["SGPRs Spill"] == 0 and r["VGPRs Spill"] == 0, name
        assert r["scratch_total"] == 0 and r["spill_in_loop"] == 0, name
