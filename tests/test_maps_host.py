"""lineal_log, elliptic and banana of ces_amd/utils.py against outputs of the reference's ces/utils.py:33-122
(tests/golden/maps.npz, written by tools/make_golden_maps.py), their place in the package, and the ABI of the map stage
(cesx_map_*, cesx_mh_run_map) as far as it goes without a GPU."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from ces_amd import models as m  # noqa: E402
from ces_amd import utils  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(GOLD, "maps.npz"))


def close(a, b, tol=1e-12):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.allclose(a, b, rtol=tol, atol=tol)


def test_lineal_log_against_the_reference(g):
    A = g["ll_A"]
    mdl = utils.lineal_log(A)
    assert (mdl.model_name, mdl.type, mdl.jacobian_adjusted, mdl.n_obs, mdl.b) == ("lineal_log", "map", True, 5, 0)
    assert close(mdl(g["ll_phi1"]), g["ll_out1"]) and close(mdl(g["ll_phiJ"]), g["ll_outJ"])
    assert close(mdl.grad_logjacobian(g["ll_phiJ"]), g["ll_grad_logjac"])
    assert close(mdl.logjacobian(g["ll_phiJ"]), g["ll_logjac"]) and close(mdl.logjacobian(g["ll_phi1"]), g["ll_logjac1"])
    mdl.jacobian_adjusted = False
    assert close(mdl.logjacobian(g["ll_phiJ"]), g["ll_logjac_off"]) and mdl.logjacobian(g["ll_phiJ"]) == 0.0
    np.random.seed(int(g["seed"]))
    noisy = utils.lineal_log(A, flag_noise=True)
    assert close(noisy(g["ll_phi1"]), g["ll_noisy1"]) and close(noisy(g["ll_phiJ"]), g["ll_noisyJ"])


def test_elliptic_against_the_reference(g):
    mdl = utils.elliptic()
    assert (mdl.model_name, mdl.type, mdl.x1, mdl.x2, mdl.sigma, mdl.flag_noise) == ("elliptic", "map", 0.25, 0.75, np.sqrt(0.01), False)
    assert repr(mdl) == str(mdl) == "elliptic"
    out = mdl(g["el_th1"])
    assert isinstance(out, list) and len(out) == 2                       # the reference returns the list [x, y]
    assert close(out, g["el_out1"]) and close(mdl(g["el_thJ"]), g["el_outJ"])
    assert close(mdl(g["el_th1"], dG=True), g["el_dG1"])
    np.random.seed(int(g["seed"]))
    assert close(utils.elliptic(flag_noise=True)(g["el_thJ"]), g["el_noisyJ"])


def test_banana_against_the_reference(g):
    mdl = utils.banana()
    assert (mdl.model_name, mdl.type, mdl.a, mdl.b, mdl.sigma) == ("banana", "map", 1.0, 0.5, np.sqrt(0.55))
    assert repr(mdl) == str(mdl) == "banana"
    th = g["bn_th"]
    assert close(mdl.Gamma, g["bn_Gamma"])
    assert close(np.stack([mdl(th[:, j]) for j in range(th.shape[1])], axis=1), g["bn_out"])
    a, b, rho = g["bn2_prm"]
    m2 = utils.banana(a=a, b=b, rho=rho)
    assert close(m2.Gamma, g["bn2_Gamma"])
    assert close(np.stack([m2(th[:, j]) for j in range(th.shape[1])], axis=1), g["bn2_out"])
    np.random.seed(int(g["seed"]))
    noisy = utils.banana(flag_noise=True)
    assert close(np.stack([noisy(th[:, j]) for j in range(th.shape[1])], axis=1), g["bn_noisy"])
    # the quirks: two normals are drawn by a noise-free call too, and a (2, J) block does not broadcast for J other than 2
    np.random.seed(int(g["seed"]))
    mdl(th[:, 0])
    assert np.random.uniform() == float(g["bn_rng_after_call"])
    with pytest.raises(ValueError):
        mdl(th[:, :3])


def test_where_the_classes_live():
    assert utils.lineal_log.engine_lineal is False and utils.lineal.engine_lineal is True
    assert issubclass(utils.lineal_log, utils.lineal)
    assert utils.elliptic().type == "map"
    import ces_amd.utils
    assert ces_amd.utils.banana is utils.banana and utils.banana.__module__ == "ces_amd.utils"
    assert not hasattr(m, "elliptic") and not hasattr(m, "banana") and not hasattr(m, "lineal_log")
    assert utils.lorenz63 is m.lorenz63                                  # the re-export of ces_amd.models still works
    for cls in (utils.elliptic, utils.banana, utils.lineal_log):
        assert callable(getattr(cls, "forward_device")) and callable(getattr(cls, "ensure_installed"))
        assert callable(getattr(cls, "invalidate_device"))
    assert utils.elliptic.fused_kind and utils.banana.fused_kind and not utils.lineal_log.fused_kind
    # (an instance too: the moments shortcut of a linear map, ShardedUpdate.lineal_fast_ok, reads it there)
    assert utils.lineal_log(np.eye(2)).engine_lineal is False


def test_device_hook_refuses_noise():
    for mdl in (utils.elliptic(flag_noise=True), utils.banana(flag_noise=True), utils.lineal_log(np.eye(2), flag_noise=True)):
        with pytest.raises(ValueError, match="noise-free"):
            mdl.forward_device(None, None)


def test_g_ens_equals_the_per_particle_loop():
    from ces_amd.calibrate import sampling
    rng = np.random.default_rng(3)
    J = 9
    U = np.vstack([rng.normal(0.0, 1.5, J), rng.uniform(90.0, 110.0, J)])
    mdl = utils.elliptic()
    G = sampling(p=2, n_obs=2, J=J).G_ens(U, mdl)
    assert G.shape == (2, J)
    assert np.array_equal(G, np.stack([np.asarray(mdl(U[:, j])) for j in range(J)], axis=1))
    A = rng.standard_normal((5, 3))
    ml = utils.lineal_log(A)
    V = rng.standard_normal((3, J))
    G = sampling(p=3, n_obs=5, J=J).G_ens(V, ml)
    assert G.shape == (5, J)
    assert np.array_equal(G, np.stack([ml(V[:, j]) for j in range(J)], axis=1))
    assert np.allclose(G, A @ np.exp(V), rtol=1e-13, atol=0.0)


@pytest.fixture(scope="module")
def lib():
    from ces_amd import build, engine
    build.build_lib()
    return engine.load_library()


def test_abi_of_the_map_stage(lib):
    from ces_amd import engine
    for name in ("cesx_map_set", "cesx_map_apply", "cesx_mh_run_map"):
        assert name in engine.EXPORTS and hasattr(lib, name)
    assert ctypes.sizeof(engine.MapDesc) == 4 + 4 + 64
    assert engine.MapDesc.prm.offset == 8
    d = engine.MapDesc()
    d.struct_bytes, d.kind = ctypes.sizeof(engine.MapDesc), engine.MAP_KINDS["elliptic"]
    # a NULL handle: the error code, no device touched
    assert lib.cesx_map_set(None, ctypes.byref(d)) == engine.EINVAL
    assert lib.cesx_map_apply(None, None, None, None) == engine.EINVAL
    assert lib.cesx_mh_run_map(None, 0, 1, 1, None, None, None, None, None) == engine.EINVAL
    assert set(engine.MAP_FUSED) == {"elliptic", "banana"} and set(engine.MAP_KINDS) == {"elliptic", "banana", "exp"}


def test_fused_on_a_model_without_a_fused_kernel():
    """``fused=True`` with ``lineal`` raises before any engine is made (no GPU here); so does ``fused=`` without ``chains=``."""
    from scipy import stats
    from ces_amd import calibrate, sample
    rng = np.random.default_rng(0)
    enka = calibrate.enka(2, 2, 10)
    enka.Ustar = rng.standard_normal((2, 10))
    mc = sample.MCMC()
    mc.mute_bar, mc.y_obs = True, np.zeros(2)
    prior = stats.multivariate_normal(mean=np.zeros(2), cov=np.identity(2))
    with pytest.raises(ValueError, match="fused"):
        mc.model_mh(utils.lineal(np.eye(2)), 3, prior, enka, np.identity(2), chains=2, fused=True)
    with pytest.raises(ValueError, match="fused"):
        mc.model_mh(utils.lineal_log(np.eye(2)), 3, prior, enka, np.identity(2), chains=2, fused=True)
    with pytest.raises(ValueError, match="fused"):
        mc.model_mh(utils.elliptic(flag_noise=True), 3, prior, enka, np.identity(2), chains=2, fused=True)
    with pytest.raises(ValueError, match="fused"):
        mc.model_mh(utils.elliptic(), 3, prior, enka, np.identity(2), fused=True)
    assert not hasattr(mc, "_mh_eng")
