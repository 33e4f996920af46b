"""The host side of the Lorenz '63 device map (ces_amd/models.py lorenz63.set_solver, device_descriptor, forward_pde_device;
sampling._device_loop_ok; MCMC.model_mh on a pde model).  No GPU needed: the engine is a stand-in that records what it is
handed."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import l63_cases as lc  # noqa: E402

W0 = np.array([-3.1, -5.2, 17.9])


def test_solve_without_set_solver_is_odeint():
    from scipy import integrate
    from ces_amd import models
    m = models.lorenz63(l_window=1, freq=10)
    t = lc.times(1.0)
    assert not hasattr(m, "forward_pde_device") and not m.solve_init
    assert np.array_equal(m.solve(W0, t, args=(27.0, 2.5)), integrate.odeint(m, W0, t, args=(27.0, 2.5)))
    ml = models.lorenz63_log(l_window=1, freq=10)
    assert np.array_equal(ml.solve(W0, t, args=(3.3, 0.9)), integrate.odeint(ml, W0, t, args=(3.3, 0.9)))


@pytest.mark.parametrize("name, args", [("lorenz63", (27.0, 2.5)), ("lorenz63_log", (3.3, 0.9))])
def test_solve_after_set_solver_is_solve_ivp(name, args):
    from scipy import integrate
    from ces_amd import models
    m = getattr(models, name)(l_window=1, freq=10)
    t = 0.5 + lc.times(2.0)                            # the span is [t[0], t[-1]], not [0, T]
    for kw in (dict(), dict(dt=0.05), dict(method="RK23", rtol=1e-5, atol=1e-8)):
        m.set_solver(**kw)
        full = dict(method="RK45", dt=np.inf, rtol=1e-3, atol=1e-6)
        full.update(kw)
        direct = integrate.solve_ivp(lambda tt, y: m(y, tt, *args), [t[0], t[-1]], W0, t_eval=t, method=full["method"],
                                     max_step=full["dt"], rtol=full["rtol"], atol=full["atol"]).y.T
        got = m.solve(W0, t, args=args)
        assert got.shape == (21, 3) and np.array_equal(got, direct)
        assert not hasattr(m, "forward_pde_device")
    with pytest.raises(ValueError, match="RK45 only"):
        m.set_solver(method="RK23", device=True)
    m.set_solver(device=True)
    assert hasattr(m, "forward_pde_device")
    m.set_solver()                                     # switching the hook off again
    assert not hasattr(m, "forward_pde_device")


def test_the_stepped_reference_is_model_solve():
    """tests/l63_cases.host_run steps scipy's RK45 itself to count the steps: bit for bit what ``model.solve`` returns."""
    for name in lc.CLASSES:
        m = lc.make_model(name, device=False)
        U, S = lc.class_params(name)
        t = lc.times(2.0)
        r = lc.host_run(m, S[:, 3], t, tuple(U[:, 3]))
        assert r["ok"] and np.array_equal(r["ws"], m.solve(S[:, 3], t, args=tuple(U[:, 3])))
        assert r["attempted"] * 6 + 2 == r["nfev"] and 0 < r["accepted"] <= r["attempted"]


@pytest.mark.parametrize("name, log", [("lorenz63", (0, 0, 0)), ("lorenz63_log", (0, 1, 1))])
def test_descriptor_of_each_class(name, log):
    m = lc.make_model(name, l_window=2, freq=5, dt=0.25, rtol=1e-4, atol=1e-7)
    t = 1.0 + np.linspace(0, 4, 21)                    # 20 samples after the first: two windows of 10
    d = m.device_descriptor(t, 2, 9)
    assert (d["n_obs"], d["p"]) == (9, 2)
    assert tuple(d["par_row"]) == (-1, 0, 1) and tuple(d["par_fixed"]) == (10.0, 0.0, 0.0) and tuple(d["par_log"]) == log
    assert (d["t0"], d["T"], d["max_step"], d["rtol"], d["atol"]) == (1.0, 5.0, 0.25, 1e-4, 1e-7)
    assert (d["window_samples"], d["max_attempts"]) == (10, 1000000)
    assert np.array_equal(d["t"], t)
    assert lc.make_model(name).device_descriptor(lc.times(1.0))["max_step"] == np.inf
    # what the descriptor says is what the class's own __call__ evaluates
    free = np.array([1.3, 0.4])
    full = [10.0] + [np.exp(v) if lg else v for v, lg in zip(free, log[1:])]
    from ces_amd import models
    assert np.array_equal(m(W0, 0.0, *free), models.lorenz63().model(W0, 0.0, *full))


def test_the_ctypes_descriptor_matches_the_header():
    from ces_amd import build, engine
    # uint32 + 3 x int32, 3 x double, 3 x int32 + pad, 5 x double, int32 + pad, pointer, int32 + pad, int64 (LP64)
    assert ctypes.sizeof(engine.L63Desc) == 16 + 24 + 16 + 40 + 8 + 8 + 8 + 8
    m = lc.make_model("lorenz63_log")
    d, keep = engine.l63_desc_struct(m.device_descriptor(lc.times(2.0), 2, 9))
    assert d.struct_bytes == ctypes.sizeof(engine.L63Desc) and d.n_t == 21 and d.t == keep.ctypes.data
    assert list(d.par_row) == [-1, 0, 1] and list(d.par_fixed) == [10.0, 0.0, 0.0] and list(d.par_log) == [0, 1, 1]
    assert (d.t0, d.T, d.max_step, d.window_samples, d.max_attempts) == (0.0, 2.0, np.inf, 10, 1000000)
    text = open(os.path.join(ROOT, "include", "cesx.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} cesx_l63_desc;", text).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = re.findall(r"(\w+)(?:\[\d+\])?\s*[,;]", body)
    assert names == [f[0] for f in engine.L63Desc._fields_]
    for name in ("cesx_lorenz_three_set", "cesx_lorenz_three_apply"):
        assert name in engine.EXPORTS and re.search(r"\b%s\s*\(" % name, text)
    assert "kernels_l63.hip" in build.SOURCES


def test_value_errors_name_the_host_path():
    t = lc.times(2.0)
    m = lc.make_model("lorenz63")
    assert m.device_descriptor(t, 2, 9)["n_obs"] == 9
    cases = [
        (dict(), dict(p=3), "p = 2 differs"),
        (dict(), dict(n_obs=8), "n_obs = 9 differs"),
        (dict(), dict(t=None), "no sample times"),
        (dict(), dict(t=t[::-1]), "must increase"),
        (dict(), dict(t=np.r_[t[:5], t[4:-1]]), "must increase"),
        (dict(), dict(t=t[:20]), "do not fill whole windows"),
        (dict(), dict(t=t[:6]), "do not fill whole windows"),
        (dict(l_window=3), dict(), "do not fill whole windows"),
        (dict(freq=2.5), dict(), "whole sample count"),
        (dict(dt=-0.1), dict(), "must be positive"),
        (dict(rtol=0.0), dict(), "must be positive"),
        (dict(atol=np.inf), dict(), "must be positive"),
        (dict(method="RK23"), dict(), "not RK45"),
    ]
    for attrs, args, what in cases:
        mm = lc.make_model("lorenz63")
        for k, v in attrs.items():
            setattr(mm, k, v)
        call = dict(t=t, p=2, n_obs=9)
        call.update(args)
        with pytest.raises(ValueError, match=what + ".*host"):
            mm.device_descriptor(call["t"], call["p"], call["n_obs"])
    host_only = lc.make_model("lorenz63", device=False)
    with pytest.raises(ValueError, match="set_solver\\(device=True\\).*host"):
        host_only.device_descriptor(t, 2, 9)


def test_the_case_table_meets_its_set_up_condition():
    """Every particle's envelope at every horizon the device tests use is below 1e-6 (measured: 3e-12 at T = 1, 4e-11 at
    T = 2, 2e-10 at T = 4), for both classes and for the fp32-rounded parameters."""
    worst = {}
    for name, T, dtype in (("lorenz63", 1, "float64"), ("lorenz63_log", 1, "float32"), ("lorenz63", 2, "float32"),
                           ("lorenz63_log", 2, "float64"), ("lorenz63_log", 4, "float64")):
        ref = lc.reference(name, T, dtype)
        worst[(name, T, dtype)] = float(ref["env"].max())
        assert ref["G"].shape == (9, lc.N_DISTINCT) and ref["W"].shape == (3, lc.N_DISTINCT)
        assert np.all(ref["accepted"] > 0) and np.all(ref["attempted"] >= ref["accepted"])
    print("l63 envelopes:", worst)
    assert max(worst.values()) <= lc.ENV_MAX
    rb, starts = lc.inputs()
    assert np.all(rb > 0) and np.all(np.abs(starts[2] - 25) < 25) and len({tuple(c) for c in starts.T}) == lc.N_DISTINCT


class _StandInEngine:
    """What ``forward_pde_device`` needs of an engine, without a device: counts the installs, keeps the token as Engine does,
    and answers ``l63_apply`` with a chosen status row."""

    def __init__(self, p, n_obs, status=(0, 0, 0)):
        self.p, self.n_obs, self.installed, self.status = p, n_obs, [], status

    def l63_set(self, desc):
        self.installed.append(desc)
        self._l63_token = object()
        return self._l63_token

    def l63_apply(self, U, W, out=None, W_out=None):
        import torch
        info = torch.zeros((4, len(self.status)), dtype=torch.int32)
        info[0] = torch.tensor(self.status, dtype=torch.int32)
        return "G", "W", info


def test_installed_once_and_again_after_a_change():
    t = lc.times(2.0)
    eng = _StandInEngine(2, 9)
    m = lc.make_model("lorenz63_log")
    assert m.forward_pde_device(eng, None, None, t) == ("G", "W") and m.forward_pde_device(eng, None, None, t) == ("G", "W")
    assert len(eng.installed) == 1
    m.forward_pde_device(eng, None, None, lc.times(1.0))                        # other sample times
    assert len(eng.installed) == 2
    m.device_max_attempts = 5
    m.forward_pde_device(eng, None, None, t)
    assert len(eng.installed) == 3 and eng.installed[-1]["max_attempts"] == 5
    m.set_solver(dt=0.05, device=True)
    m.forward_pde_device(eng, None, None, t)
    assert len(eng.installed) == 4 and eng.installed[-1]["max_step"] == 0.05
    other = lc.make_model("lorenz63_log")
    other.forward_pde_device(eng, None, None, t)
    m.forward_pde_device(eng, None, None, t)                                    # another model installed its map in between
    assert len(eng.installed) == 6
    m.invalidate_device()
    m.forward_pde_device(eng, None, None, t)
    assert len(eng.installed) == 7
    wrong = _StandInEngine(3, 9)
    with pytest.raises(ValueError, match="p = 2 differs"):
        m.forward_pde_device(wrong, None, None, t)
    assert not wrong.installed


def test_check_false_reads_no_status():
    """``check=True`` (default) raises on a failed particle, naming it; ``check=False`` returns what the engine returned --
    for this hook and for Lorenz '96's."""
    import l96_cases as l96
    t = lc.times(2.0)
    m = lc.make_model("lorenz63")
    for status, text in ((1, "step size"), (2, "not finite"), (3, "max_attempts")):
        eng = _StandInEngine(2, 9, status=(0, 0, status, 2))
        with pytest.raises(ValueError, match="particle 2 failed with status %d.*%s" % (status, text)):
            m.forward_pde_device(eng, None, None, t)
        with pytest.raises(ValueError, match="particle 2 failed"):
            m.forward_pde_device(eng, None, None, t, check=True)
        assert m.forward_pde_device(eng, None, None, t, check=False) == ("G", "W")

    class _L96Engine(_StandInEngine):
        def l96_set(self, desc):
            self.installed.append(desc)
            self._l96_token = object()
            return self._l96_token
        l96_apply = _StandInEngine.l63_apply
    m96 = l96.make_model("lorenz96Fb", (5, 3), T=0.2)
    eng = _L96Engine(2, 25, status=(0, 3))
    with pytest.raises(ValueError, match="particle 1 failed with status 3"):
        m96.forward_pde_device(eng, None, None, l96.times(0.2))
    assert m96.forward_pde_device(eng, None, None, l96.times(0.2), check=False) == ("G", "W")


def test_device_loop_ok_on_a_lorenz63_model():
    from ces_amd.calibrate import sampling
    eks = sampling(p=2, n_obs=9, J=8)
    eks.noise = "device"
    with_hook, without = lc.make_model("lorenz63_log"), lc.make_model("lorenz63_log", device=False)
    assert eks._device_loop_ok(with_hook, False, {})
    assert not eks._device_loop_ok(without, False, {})
    assert not eks._device_loop_ok(with_hook, False, dict(ws=np.zeros((3, 3))))
    eks.noise = "numpy"
    assert not eks._device_loop_ok(with_hook, False, {}) and eks._device_loop_ok(with_hook, False, dict(xis=[None]))


def test_host_model_mh_runs_a_pde_model_after_set_solver():
    """The reference's notebook ends in ``model_mh`` on the true model; after ``set_solver`` the host sampler integrates with
    ``solve_ivp``: every kept state's phi is reproduced from ``solve`` + ``statistics``."""
    from scipy import stats
    from ces_amd import calibrate, sample
    m = lc.make_model("lorenz63_log", device=False)
    m.t, m.wt = lc.times(2.0), np.array(lc.attractor_states()[:, 0])
    truth = np.log([28.0, 8.0 / 3])
    y = m.statistics(m.solve(m.wt, m.t, args=tuple(truth)))
    Gamma = np.diag((0.05 * np.abs(y) + 0.1) ** 2)
    prior = stats.multivariate_normal(mean=truth, cov=0.04 * np.eye(2))
    enka = calibrate.enka(2, 9, 16)
    enka.Ustar = truth[:, None] + 0.02 * np.random.RandomState(0).standard_normal((2, 16))
    mc = sample.MCMC()
    mc.mute_bar, mc.y_obs = True, y
    np.random.seed(5)
    mc.model_mh(m, 6, prior, enka, Gamma)
    assert mc.samples.shape == (2, 7) and np.all(np.isfinite(mc.samples)) and 0.0 <= mc.accept <= 1.0
    assert np.array_equal(mc.samples[:, 0], enka.Ustar.mean(axis=1))
    # the forward map it ran is solve_ivp's: G_pde of a kept state, from the model's own pieces
    g = enka.G_pde(np.hstack([mc.samples[:, -1], m.wt]), m, m.t)
    ws = m.solve(m.wt, m.t, args=tuple(mc.samples[:, -1]))
    assert np.array_equal(g, np.concatenate([m.statistics(ws), ws[-1]]))


def test_l63_kernels_have_no_scratch_and_no_lds():
    import isa_audit
    t = isa_audit.collect(["kernels_l63.hip"])
    names = isa_audit.demangle(sorted(t))
    rows = {names[k]: v for k, v in t.items() if "l63_kernel" in names[k]}
    assert len(rows) == 2                                    # float, double
    for name, r in rows.items():
        assert r["ScratchSize [bytes/lane]"] == 0 and r["scratch_total"] == 0 and r["VGPRs Spill"] == 0, name
        assert r["LDS Size [bytes/block]"] == 0, name
