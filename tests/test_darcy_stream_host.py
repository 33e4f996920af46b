"""The host side of the streamed Darcy device map (``model.set_device_solver('streamed')``; no GPU needed).

The cases' conditioning and sign structure, the streamed descriptor applied in numpy (``darcy_cases.apply_descriptor``: the
algorithm the kernel implements) against the host map to the bound the GPU tests hold the kernel to
(tests/test_gpu_darcy_stream.py), the ValueError cases, the re-install on a change of solver, the ABI and the new kernel's
registers.
"""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import darcy_cases as dc  # noqa: E402
import darcy_stream_cases as sc  # noqa: E402


@pytest.mark.parametrize("shape", list(sc.SHAPES), ids=sc.SHAPE_IDS)
def test_every_shape_is_conditioned_and_exercises_the_pivoting_path(shape):
    """Every particle of every case stays below the conditioning where the parity bound still means something and has a
    finite host value, in fp64 and at the fp32-rounded inputs; every shape but (64, 64, 50) -- which is about sizes -- has
    particles with a non-positive nodal coefficient among its scales (A is indefinite there: the LU pivots)."""
    for dtype in ("float64", "float32"):
        refs = [sc.reference(*shape, scale, dtype) for scale in sc.SCALES]
        assert all(r["G"].shape == (shape[2], sc.SHAPES[shape]) for r in refs)
        assert max(float(r["cond"].max()) for r in refs) < sc.COND_MAX
        assert all(np.all(np.isfinite(r["G"])) for r in refs)
        if shape != (64, 64, 50):
            assert sum(int(np.sum(r["amin"] <= 0.0)) for r in refs) >= 1


def test_shared_shape_is_the_existing_reference():
    """(16, 256, 50) is ``darcy_cases``' own case: the same draw, the same host values, its leading columns."""
    a, b = sc.reference(16, 256, 50, 3, "float32"), dc.reference(16, 256, 50, 3, "float32")
    assert np.array_equal(a["U"], b["U"][:, :32]) and np.array_equal(a["G"], b["G"][:, :32])
    # and a shape of this module's own follows the same recipe
    K, p, n_obs, scale = 17, 20, 9, 10
    rng = np.random.default_rng(300000 + 1000 * K + 10 * p + scale)
    U = (scale * rng.standard_normal((p, 130))).astype("float32").astype(np.float64)
    ref = sc.reference(K, p, n_obs, scale, "float32")
    assert np.array_equal(ref["U"], U[:, :32]) and np.array_equal(ref["G"][:, 5], ref["model"](U[:, 5]))


@pytest.mark.parametrize("scale", sc.SCALES)
@pytest.mark.parametrize("shape", list(sc.SHAPES), ids=sc.SHAPE_IDS)
def test_streamed_descriptor_on_the_cpu(shape, scale):
    K, p, n_obs = shape
    ref = sc.reference(K, p, n_obs, scale, "float64")
    mdl = sc.make_model(K, p, n_obs)
    desc = mdl.device_descriptor(n_obs)
    assert desc["solver"] == "streamed" and desc["max_workgroups"] == 0
    assert desc["K"] == K and desc["scatter"].shape == (p,) and desc["obs_index"].shape == (n_obs,)
    J = sc.SHAPES[shape]
    G = np.stack([dc.apply_descriptor(desc, ref["U"][:, j]) for j in range(J)], axis=1)
    ratio = sc.check(G, ref, "float64", (shape, scale))
    print("\n[darcy-stream] restatement, %s scale %d: %.3g of the bound's 16" % (shape, scale, ratio))
    # the arrays are the resident descriptor's
    res = sc.make_model(K, p, n_obs, solver=None)
    if K <= 16:
        d0 = res.device_descriptor(n_obs)
        assert "solver" not in d0 and "max_workgroups" not in d0
        assert all(np.array_equal(d0[k], desc[k]) for k in d0)


class _StandInEngine:
    def __init__(self, p, n_obs):
        self.p, self.n_obs, self.installed = p, n_obs, []

    def darcy_set(self, desc):
        self.installed.append(desc)
        self._darcy_token = object()
        return self._darcy_token

    def darcy_apply(self, U, out=None):
        return "G"


def test_set_device_solver_errors():
    from ces_amd import darcy
    mdl = darcy.model_trunc(Nmesh=32.0, p=4)
    mdl.obs_index = np.arange(12)
    assert mdl.device_solver == "resident" and mdl.device_max_workgroups == 0
    for bad in ("Streamed", "hbm", None, 1):
        with pytest.raises(ValueError, match="neither 'resident' nor 'streamed'"):
            mdl.set_device_solver(bad)
    assert mdl.device_solver == "resident"
    eng = _StandInEngine(4, 12)
    # without a call, Nmesh = 32 raises as before (the text tests/test_darcy_device_host.py matches, then the hint)
    with pytest.raises(ValueError, match=r"Nmesh = 32 > 16 is not supported on the device; evaluate the map on the host "
                                         r"\(model\(xi\), enka\.G_ens\) instead.*set_device_solver\('streamed'\)"):
        mdl.forward_device(eng, None)
    assert not eng.installed
    mdl.set_device_solver("streamed")
    assert mdl.forward_device(eng, None) == "G" and eng.installed[-1]["K"] == 32 and eng.installed[-1]["solver"] == "streamed"
    big = darcy.model_trunc(Nmesh=65.0, p=4)
    big.obs_index = np.arange(12)
    big.set_device_solver("streamed")
    with pytest.raises(ValueError, match="Nmesh = 65 > 64.*host"):
        big.forward_device(eng, None)
    small = darcy.model_trunc(Nmesh=3.0, p=4)
    small.obs_index = np.arange(12) % 9
    small.set_device_solver("streamed")
    with pytest.raises(ValueError, match="< 4.*host"):
        small.forward_device(eng, None)
    assert len(eng.installed) == 1
    at = darcy.model_trunc(Nmesh=64.0, p=4)
    at.obs_index = np.arange(12)
    at.set_device_solver("streamed")
    at.device_max_workgroups = 7
    d = at.device_descriptor(12)
    assert d["K"] == 64 and d["max_workgroups"] == 7


def test_installed_once_and_again_after_the_solver_changes():
    from ces_amd import darcy
    eng = _StandInEngine(10, 12)
    mdl = darcy.model_trunc(Nmesh=8.0, p=10)
    mdl.obs_index = np.arange(12)
    assert mdl.forward_device(eng, None) == "G" and mdl.forward_device(eng, None) == "G"
    assert len(eng.installed) == 1 and "solver" not in eng.installed[0]
    mdl.set_device_solver("streamed")
    mdl.forward_device(eng, None)
    mdl.forward_device(eng, None)
    assert len(eng.installed) == 2 and eng.installed[1]["solver"] == "streamed"
    mdl.set_device_solver("streamed")                        # the same kind again: nothing to install
    mdl.forward_device(eng, None)
    assert len(eng.installed) == 2
    mdl.device_max_workgroups = 3
    mdl.forward_device(eng, None)
    assert len(eng.installed) == 3 and eng.installed[2]["max_workgroups"] == 3
    mdl.set_device_solver("resident")
    mdl.forward_device(eng, None)
    assert len(eng.installed) == 4 and "solver" not in eng.installed[3]


def test_abi_declares_and_exports_the_entry_points():
    from ces_amd import build, engine
    text = open(os.path.join(ROOT, "include", "cesx.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = set(re.findall(r"\b(cesx_[a-z_]+)\s*\(", code))
    for name in ("cesx_darcy_set_streamed", "cesx_darcy_workspace_bytes"):
        assert name in names and name in engine.EXPORTS
    assert "#define CESX_ABI_VERSION %d" % engine.ABI_VERSION in code and engine.ABI_VERSION >= 6
    assert "#define CESX_DARCY_STREAM_KMAX 64" in code
    assert "kernels_darcy_stream.hip" in build.SOURCES
    build.build_lib()
    lib = engine.load_library()
    assert hasattr(lib, "cesx_darcy_set_streamed") and hasattr(lib, "cesx_darcy_workspace_bytes")
    assert lib.cesx_abi_version() == engine.ABI_VERSION
    from ces_amd import darcy
    assert darcy.model.DEVICE_NMESH_STREAMED == (4, 64) and darcy.model.DEVICE_NMESH == (4, 16)


def test_streamed_kernels_have_no_scratch_and_no_spills():
    import isa_audit
    t = isa_audit.collect(["kernels_darcy_stream.hip"])
    names = isa_audit.demangle(sorted(t))
    rows = {names[k]: v for k, v in t.items() if "darcy_stream_lu" in names[k]}
    assert len(rows) == 2                                    # float, double
    assert not any("darcy_kernel" in names[k] for k in t)
    for name, r in rows.items():
        assert r["ScratchSize [bytes/lane]"] == 0 and r["scratch_total"] == 0, name
        assert r["SGPRs Spill"] == 0 and r["VGPRs Spill"] == 0 and r["spill_total"] == 0, name
