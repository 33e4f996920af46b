"""The host side of the Darcy device map (ces_amd/darcy.py device_descriptor / forward_device; no GPU needed).

The descriptor ``forward_device`` hands the engine is applied in numpy, with ``scipy.linalg.solve_banded`` (partial-pivot
banded LU) as the solver, and must reproduce the host map ``model(k)`` to the bound the GPU tests hold the kernel to
(tests/test_gpu_darcy.py): this pins the matrices, the scatter, the flatten order and the column-major reshape independently
of the kernel.  Also: the cases' conditioning and sign structure, the ValueError cases, the ABI and the kernels' registers.
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

SHAPE_IDS = ["K%d-p%d-n%d" % s for s in dc.SHAPES]


@pytest.mark.parametrize("shape", dc.SHAPES, ids=SHAPE_IDS)
def test_every_shape_exercises_the_pivoting_path(shape):
    """From the HOST's nodal coefficients: each (K, p) has particles with a non-positive nodal coefficient among its scale
    cases (A is indefinite there and a Cholesky would fail), in fp64 and at the fp32-rounded inputs -- and every particle of
    every case stays below the conditioning where the parity bound still means something."""
    for dtype in ("float64", "float32"):
        refs = [dc.reference(*shape, scale, dtype) for scale in dc.SCALES]
        assert sum(int(np.sum(r["amin"] <= 0.0)) for r in refs) >= 1
        assert max(float(r["cond"].max()) for r in refs) < dc.COND_MAX
        assert all(np.all(np.isfinite(r["G"])) for r in refs)


@pytest.mark.parametrize("scale", dc.SCALES)
@pytest.mark.parametrize("shape", dc.SHAPES, ids=SHAPE_IDS)
def test_descriptor_on_the_cpu(shape, scale):
    K, p, n_obs = shape
    ref = dc.reference(K, p, n_obs, scale, "float64")
    mdl = dc.make_model(K, p, n_obs)
    desc = mdl.device_descriptor(n_obs)
    assert desc["K"] == K and desc["scatter"].shape == (p,) and desc["obs_index"].shape == (n_obs,)
    J = 33
    G = np.stack([dc.apply_descriptor(desc, ref["U"][:, j]) for j in range(J)], axis=1)
    tol, gmax, cond = dc.tolerance(ref, "float64", J)
    err = np.max(np.abs(G - ref["G"][:, :J]), axis=0)
    assert np.all(err <= tol), (err / tol).max()
    # picked entries of the full solution, in the host's flatten order
    full = mdl(ref["U"][:, 0], full_solution=True)
    assert np.array_equal(full[mdl.obs_index], ref["G"][:, 0])


def test_descriptor_matrices_are_the_modules_own_operators():
    from ces_amd import darcy
    K = 7
    mdl = darcy.model(Nmesh=float(K))
    mdl.obs_index = np.arange(3)
    d = mdl.device_descriptor(3)
    rng = np.random.default_rng(0)
    z = rng.standard_normal((K, K))
    centres, nodes = np.arange(1, 2 * K, 2) / (2.0 * K), np.linspace(0.0, 1.0, K)
    assert np.allclose(d["S"] @ z @ d["S"].T, darcy._interp2_spline(centres, z, nodes), rtol=0, atol=1e-12 * np.abs(z).max() * 50)
    assert np.allclose(d["R"] @ z @ d["R"].T, darcy._interp2_spline(nodes, z, centres), rtol=0, atol=1e-12)
    xi = rng.standard_normal(K * K)
    L = d["coef"] * xi.reshape(K, K)
    assert L[0, 0] == 0.0
    assert np.allclose(d["D"] @ L @ d["D"].T, mdl.eval_rf(xi), rtol=0, atol=1e-13)
    assert np.array_equal(d["scatter"], np.arange(K * K))
    t = darcy.model_trunc(Nmesh=float(K), p=9)
    t.obs_index = np.arange(3)
    assert np.array_equal(t.device_descriptor()["scatter"], t.rank[:9])


class _StandInEngine:
    """What ``forward_device`` needs of an engine, without a device: counts the installs, keeps the token as Engine does."""

    def __init__(self, p, n_obs):
        self.p, self.n_obs, self.installed = p, n_obs, []

    def darcy_set(self, desc):
        self.installed.append(desc)
        self._darcy_token = object()
        return self._darcy_token

    def darcy_apply(self, U, out=None):
        return "G"


def test_value_errors_name_the_host_path():
    from ces_amd import darcy
    eng = _StandInEngine(10, 12)
    mdl = darcy.model_trunc(Nmesh=8.0, p=10)
    with pytest.raises(ValueError, match="obs_index is not set.*host"):
        mdl.forward_device(eng, None)
    mdl.obs_index = np.arange(11)
    with pytest.raises(ValueError, match="len\\(obs_index\\) = 11 differs.*host"):
        mdl.forward_device(eng, None)
    for nmesh, what in ((3.0, "< 4"), (32.0, "> 16")):
        m = darcy.model_trunc(Nmesh=nmesh, p=4)
        m.obs_index = np.arange(12) % 9
        e4 = _StandInEngine(4, 12)
        with pytest.raises(ValueError, match=what + ".*host"):
            m.forward_device(e4, None)
        assert not e4.installed
    mdl.obs_index = np.arange(12)
    mdl.p = 9
    with pytest.raises(ValueError, match="p = 9 differs"):
        mdl.forward_device(eng, None)
    assert not eng.installed


def test_installed_once_and_again_after_a_change():
    from ces_amd import darcy
    eng = _StandInEngine(10, 12)
    mdl = darcy.model_trunc(Nmesh=8.0, p=10)
    mdl.obs_index = np.arange(12)
    assert mdl.forward_device(eng, None) == "G" and mdl.forward_device(eng, None) == "G"
    assert len(eng.installed) == 1
    mdl.obs_index = np.arange(12)[::-1].copy()
    mdl.forward_device(eng, None)
    assert len(eng.installed) == 2 and np.array_equal(eng.installed[-1]["obs_index"], np.arange(12)[::-1])
    mdl.tau = 2.0
    mdl.forward_device(eng, None)
    assert len(eng.installed) == 3
    other = darcy.model_trunc(Nmesh=8.0, p=10)
    other.obs_index = np.arange(12)
    other.forward_device(eng, None)
    mdl.forward_device(eng, None)                          # another model installed its map in between
    assert len(eng.installed) == 5
    mdl.invalidate_device()
    mdl.forward_device(eng, None)
    assert len(eng.installed) == 6


def test_host_path_is_unchanged_by_the_hook():
    """``__call__`` does not look at the device state."""
    from ces_amd import darcy
    mdl = dc.make_model(8, 10, 12)
    xi = np.random.default_rng(1).standard_normal(10)
    before = mdl(xi)
    mdl.invalidate_device()
    mdl.device_descriptor(12)
    assert np.array_equal(mdl(xi), before)
    assert hasattr(darcy.model, "forward_device") and not hasattr(darcy.model, "engine_lineal")


def test_replaced_hooks_keep_the_plain_loop():
    """A caller that replaced G_ens or an update hook on the instance gets the loop that calls them (the benchmark's Darcy
    leg times the host map that way); otherwise a Darcy model now qualifies for the device-resident loop."""
    from ces_amd.calibrate import sampling
    mdl = dc.make_model(8, 10, 12)
    eks = sampling(p=10, n_obs=12, J=8)
    eks.noise = "device"
    assert eks._device_loop_ok(mdl, False, {})
    eks.noise = "numpy"
    assert not eks._device_loop_ok(mdl, False, {}) and eks._device_loop_ok(mdl, False, dict(xis=[None]))
    eks.noise = "device"
    eks.G_ens = lambda theta, m: None
    assert not eks._device_loop_ok(mdl, False, {})
    del eks.G_ens
    eks.eks_update_aldi = lambda *a, **k: None
    assert not eks._device_loop_ok(mdl, False, {})


def _declared():
    text = open(os.path.join(ROOT, "include", "cesx.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(cesx_[a-z_]+)\s*\(", text)), text


def test_abi_declares_and_exports_the_entry_points():
    import ctypes
    from ces_amd import build, engine
    names, text = _declared()
    for name in ("cesx_darcy_set", "cesx_darcy_apply"):
        assert name in names and name in engine.EXPORTS
    assert "cesx_darcy_desc" in text and "#define CESX_ABI_VERSION %d" % engine.ABI_VERSION in text and engine.ABI_VERSION >= 3
    assert "kernels_darcy.hip" in build.SOURCES
    build.build_lib()
    lib = engine.load_library()
    assert hasattr(lib, "cesx_darcy_set") and hasattr(lib, "cesx_darcy_apply")
    # uint32 + 3 x int32, then six pointers (LP64)
    assert ctypes.sizeof(engine.DarcyDesc) == 16 + 6 * 8


def test_darcy_kernels_have_no_scratch_and_no_spills():
    import isa_audit
    t = isa_audit.collect(["kernels_darcy.hip"])
    names = isa_audit.demangle(sorted(t))
    rows = {names[k]: v for k, v in t.items() if "darcy_kernel" in names[k]}
    assert len(rows) == 2                                    # float, double
    for name, r in rows.items():
        assert r["ScratchSize [bytes/lane]"] == 0 and r["scratch_total"] == 0, name
        assert r["SGPRs Spill"] == 0 and r["VGPRs Spill"] == 0 and r["spill_total"] == 0, name
