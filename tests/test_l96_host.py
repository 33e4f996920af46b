"""The host side of the Lorenz '96 device map (ces_amd/models.py set_solver(device=True), device_descriptor,
forward_pde_device; sampling._device_loop_ok).  No GPU needed: the engine is a stand-in that records what it is handed."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import l96_cases as lc  # noqa: E402

LOG10 = np.log(10)


def test_device_false_leaves_the_model_as_it_was():
    from ces_amd import models
    a, b, c = models.lorenz96(5, 3), models.lorenz96(5, 3), models.lorenz96(5, 3)
    a.set_solver(T=0.2, dt=0.1)
    b.set_solver(T=0.2, dt=0.1, device=False)
    assert vars(a) == vars(b) and not hasattr(a, "forward_pde_device")
    assert sorted(vars(a)) == sorted(["n_slow", "n_fast", "n_state", "l_window", "freq", "spinup", "solve_init", "model_name",
                                      "type", "method", "dt", "T"])
    c.set_solver(T=0.2, dt=0.1, device=True)
    assert hasattr(c, "forward_pde_device")
    w0 = lc.attractor_state(5, 3)
    t = lc.times(0.2)
    assert np.array_equal(a.solve(w0, t, args=tuple(lc.PAR_MEAN)), c.solve(w0, t, args=tuple(lc.PAR_MEAN)))
    c.set_solver(T=0.2, dt=0.1)                        # switching the hook off again
    assert vars(a) == vars(c)
    with pytest.raises(ValueError, match="RK45 only"):
        a.set_solver(method="RK23", device=True)
    a.set_solver(method="RK23")                        # the host path takes any method, as before
    assert a.method == "RK23"


def test_the_stepped_reference_is_model_solve():
    """tests/l96_cases.host_run steps scipy's RK45 itself to count the steps: bit for bit what ``model.solve`` returns."""
    m = lc.make_model("lorenz96", (5, 3), T=0.2, device=False)
    U, S = lc.class_params("lorenz96", (5, 3))
    t = lc.times(0.2)
    r = lc.host_run(m, S[:, 3], t, tuple(U[:, 3]))
    assert r["ok"] and np.array_equal(r["ws"], m.solve(S[:, 3], t, args=tuple(U[:, 3])))
    assert r["attempted"] * 6 + 2 == r["nfev"] and 0 < r["accepted"] <= r["attempted"]


@pytest.mark.parametrize("name, row, fixed, mode, n_obs, p", [
    ("lorenz96", (0, 1, 2, 3), (0., 0., 0., 0.), 0, 25, 4),
    ("lorenz96_hom", (0, 1, 2, 3), (0., 0., 0., 0.), 1, 5, 4),
    ("lorenz96Fc", (-1, 0, 1, -1), (1., 0., 0., 10.), 0, 180, 2),
    ("lorenz96Fb", (-1, 0, -1, 1), (1., 0., LOG10, 0.), 0, 25, 2),
    ("lorenz96hFb", (0, 1, -1, 2), (0., 0., LOG10, 0.), 0, 25, 3),
    ("lorenz96hcb", (0, -1, 1, 2), (0., 10., 0., 0.), 0, 25, 3),
])
def test_descriptor_of_each_class(name, row, fixed, mode, n_obs, p):
    m = lc.make_model(name, (5, 3), T=4, dt=0.1, l_window=2, freq=10, spinup=1)
    t = np.linspace(0, 4, 51)                          # 50 samples after the first: 10 of spin-up, two windows of 20
    if name == "lorenz96_hom":
        n_obs = 5
    d = m.device_descriptor(t, p, n_obs)
    ns, nf = lc.model_shape(name, (5, 3))
    assert (d["n_slow"], d["n_fast"], d["n_obs"], d["p"], d["stat_mode"]) == (ns, nf, n_obs, p, mode)
    assert tuple(d["par_row"]) == row and tuple(d["par_fixed"]) == fixed
    assert (d["T"], d["max_step"], d["rtol"], d["atol"]) == (4.0, 0.1, 1e-3, 1e-6)
    assert (d["spinup_samples"], d["window_samples"], d["max_attempts"]) == (10, 20, 1000000)
    assert np.array_equal(d["t"], t)
    # the fixed values are the defaults of the class's own __call__: the host evaluates the same right-hand side
    w = lc.attractor_state(ns, nf)
    free = np.array([0.7, 9.0, 2.0, 8.0])[[s for s in range(4) if row[s] >= 0]]
    full = [free[row[s]] if row[s] >= 0 else fixed[s] for s in range(4)]
    assert np.array_equal(m(0.0, w, *free), m.model(w, 0.0, *full))
    if name == "lorenz96_hom":
        m.hom = False
        assert m.device_descriptor(t, p, 5)["stat_mode"] == 2


def test_the_ctypes_descriptor_matches_the_header():
    from ces_amd import engine
    # uint32 + 5 x int32, 4 x int32, 4 x double, 4 x double, int32 + pad, pointer, 2 x int32, int64 (LP64)
    assert ctypes.sizeof(engine.L96Desc) == 24 + 16 + 32 + 32 + 8 + 8 + 8 + 8
    m = lc.make_model("lorenz96Fb", (5, 3), T=0.2)
    d, keep = engine.l96_desc_struct(m.device_descriptor(lc.times(0.2), 2, 25))
    assert d.struct_bytes == ctypes.sizeof(engine.L96Desc) and d.n_t == 21 and d.t == keep.ctypes.data
    assert list(d.par_row) == [-1, 0, -1, 1] and list(d.par_fixed) == [1.0, 0.0, LOG10, 0.0] and d.max_attempts == 1000000
    text = open(os.path.join(ROOT, "include", "cesx.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} cesx_l96_desc;", text).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = re.findall(r"(\w+)(?:\[\d+\])?\s*[,;]", body)
    assert names == [f[0] for f in engine.L96Desc._fields_]
    for name in ("cesx_lorenz_set", "cesx_lorenz_apply"):
        assert name in engine.EXPORTS and re.search(r"\b%s\s*\(" % name, text)
    from ces_amd import build
    assert "kernels_l96.hip" in build.SOURCES


def test_value_errors_name_the_host_path():
    t = lc.times(0.2)
    m = lc.make_model("lorenz96", (5, 3), T=0.2)
    ok = m.device_descriptor(t, 4, 25)
    assert ok["n_obs"] == 25
    cases = [
        (dict(), dict(p=3), "p = 4 differs"),
        (dict(), dict(n_obs=24), "n_obs = 25 differs"),
        (dict(), dict(t=None), "no sample times"),
        (dict(), dict(t=t[::-1]), "must increase"),
        (dict(), dict(t=t * 2), "must increase within"),
        (dict(), dict(t=np.r_[-0.01, t[1:]]), "must increase within"),
        (dict(), dict(t=t[:20]), "do not fill whole windows"),
        (dict(spinup=2), dict(), "do not fill whole windows"),
        (dict(l_window=3), dict(), "do not fill whole windows"),
        (dict(freq=2.5), dict(), "whole sample counts"),
        (dict(T=0.0), dict(), "must be positive"),
        (dict(dt=-0.1), dict(), "must be positive"),
        (dict(n_slow=3, n_state=12), dict(n_obs=15), "n_slow = 3 < 4"),
        (dict(n_fast=0, n_state=5), dict(), "n_fast = 0 < 1"),
        (dict(n_slow=50, n_fast=10), dict(n_obs=250), "n_state = 550 > 448"),
        (dict(method="RK23"), dict(), "not RK45"),
    ]
    for attrs, args, what in cases:
        mm = lc.make_model("lorenz96", (5, 3), T=0.2)
        for k, v in attrs.items():
            setattr(mm, k, v)
        call = dict(t=t, p=4, n_obs=25)
        call.update(args)
        with pytest.raises(ValueError, match=what + ".*host"):
            mm.device_descriptor(call["t"], call["p"], call["n_obs"])
    host_only = lc.make_model("lorenz96", (5, 3), T=0.2, device=False)
    with pytest.raises(ValueError, match="set_solver\\(device=True\\).*host"):
        host_only.device_descriptor(t, 4, 25)
    hom = lc.make_model("lorenz96_hom", None, T=0.2)
    hom.hom, hom.n_slow, hom.n_fast = False, 7, 3
    with pytest.raises(ValueError, match="slow index 7.*host"):
        hom.device_descriptor(t, 4, 5)


class _StandInEngine:
    """What ``forward_pde_device`` needs of an engine, without a device: counts the installs, keeps the token as Engine does,
    and answers ``l96_apply`` with a chosen status row."""

    def __init__(self, p, n_obs, status=(0, 0, 0)):
        self.p, self.n_obs, self.installed, self.status = p, n_obs, [], status

    def l96_set(self, desc):
        self.installed.append(desc)
        self._l96_token = object()
        return self._l96_token

    def l96_apply(self, U, W, out=None, W_out=None):
        import torch
        info = torch.zeros((4, len(self.status)), dtype=torch.int32)
        info[0] = torch.tensor(self.status, dtype=torch.int32)
        return "G", "W", info


def test_installed_once_and_again_after_a_change():
    t = lc.times(0.2)
    eng = _StandInEngine(2, 25)
    m = lc.make_model("lorenz96Fb", (5, 3), T=0.2)
    assert m.forward_pde_device(eng, None, None, t) == ("G", "W") and m.forward_pde_device(eng, None, None, t) == ("G", "W")
    assert len(eng.installed) == 1
    m.forward_pde_device(eng, None, None, lc.times(0.2, t_last=0.15))          # other sample times
    assert len(eng.installed) == 2
    m.device_max_attempts = 5
    m.forward_pde_device(eng, None, None, t)
    assert len(eng.installed) == 3 and eng.installed[-1]["max_attempts"] == 5
    m.set_solver(T=0.2, dt=0.05, device=True)
    m.forward_pde_device(eng, None, None, t)
    assert len(eng.installed) == 4 and eng.installed[-1]["max_step"] == 0.05
    other = lc.make_model("lorenz96Fb", (5, 3), T=0.2)
    other.forward_pde_device(eng, None, None, t)
    m.forward_pde_device(eng, None, None, t)                                    # another model installed its map in between
    assert len(eng.installed) == 6
    m.invalidate_device()
    m.forward_pde_device(eng, None, None, t)
    assert len(eng.installed) == 7
    wrong = _StandInEngine(3, 25)
    with pytest.raises(ValueError, match="p = 2 differs"):
        m.forward_pde_device(wrong, None, None, t)
    assert not wrong.installed


def test_a_failed_particle_raises_value_error_naming_the_column():
    t = lc.times(0.2)
    m = lc.make_model("lorenz96Fb", (5, 3), T=0.2)
    for status, text in ((1, "step size"), (2, "not finite"), (3, "max_attempts")):
        eng = _StandInEngine(2, 25, status=(0, 0, status, 2))
        with pytest.raises(ValueError, match="particle 2 failed with status %d.*%s" % (status, text)):
            m.forward_pde_device(eng, None, None, t)


def test_device_loop_ok_on_a_pde_model():
    from ces_amd.calibrate import sampling
    eks = sampling(p=2, n_obs=25, J=8)
    eks.noise = "device"
    with_hook = lc.make_model("lorenz96Fb", (5, 3), T=0.2)
    without = lc.make_model("lorenz96Fb", (5, 3), T=0.2, device=False)
    assert eks._device_loop_ok(with_hook, False, {})
    assert not eks._device_loop_ok(without, False, {})
    assert not eks._device_loop_ok(with_hook, False, dict(ws=np.zeros((3, 20))))
    assert not eks._device_loop_ok(with_hook, True, {})
    eks.noise = "numpy"
    assert not eks._device_loop_ok(with_hook, False, {}) and eks._device_loop_ok(with_hook, False, dict(xis=[None]))
    assert not eks._device_loop_ok(with_hook, False, dict(xis=[None], ws=np.zeros((3, 20))))
    eks.G_ens = lambda theta, m: None
    assert not eks._device_loop_ok(with_hook, False, dict(xis=[None]))


def test_l96_kernels_have_no_scratch():
    import isa_audit
    t = isa_audit.collect(["kernels_l96.hip"])
    names = isa_audit.demangle(sorted(t))
    rows = {names[k]: v for k, v in t.items() if "l96_kernel" in names[k]}
    assert len(rows) == 8                                    # float, double x 1, 2, 4, 7 lane stripes
    for name, r in rows.items():
        assert r["ScratchSize [bytes/lane]"] == 0 and r["scratch_total"] == 0 and r["VGPRs Spill"] == 0, name
