"""Write tests/golden/maps.npz: inputs and the REFERENCE's outputs for lineal_log, elliptic and banana (ces/utils.py:33-122).

Loads the real reference through ``oracle._refload.load_reference_utils()`` (read-only; runs only where the reference
exists) and records, for each of the three maps: single particles and -- where the reference accepts them -- (p, J)
blocks, ``dG=True``, both Jacobian helpers, ``banana().Gamma`` and the ``flag_noise=True`` outputs under a recorded
``np.random.seed``.  Data only, a few KB.  tests/test_maps_host.py replays every call against ces_amd.utils.

    python tools/make_golden_maps.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED = 20240607


def main():
    from oracle._refload import load_reference_utils
    ref = load_reference_utils()
    rng = np.random.default_rng(7)
    out = {"seed": np.array(SEED)}

    # ---- lineal_log: (n, p) = (5, 3); one particle, a (p, J) block, both helpers, the seeded noisy call ----
    A = rng.standard_normal((5, 3))
    phi1 = rng.standard_normal(3)
    phiJ = rng.standard_normal((3, 6))
    m = ref.lineal_log(A)
    out.update(ll_A=A, ll_phi1=phi1, ll_phiJ=phiJ, ll_out1=m(phi1), ll_outJ=m(phiJ),
               ll_grad_logjac=m.grad_logjacobian(phiJ), ll_logjac=np.asarray(m.logjacobian(phiJ)),
               ll_logjac1=np.asarray(m.logjacobian(phi1)))
    m.jacobian_adjusted = False
    out["ll_logjac_off"] = np.asarray(m.logjacobian(phiJ))
    np.random.seed(SEED)
    noisy = ref.lineal_log(A, flag_noise=True)
    out["ll_noisy1"] = noisy(phi1)
    out["ll_noisyJ"] = noisy(phiJ)

    # ---- elliptic: the notebook's ranges (u1 around -3 .. 3, u2 around 90 .. 110) ----
    th1 = np.array([-2.7, 104.5])
    thJ = np.vstack([rng.uniform(-3.0, 3.0, 7), rng.uniform(90.0, 110.0, 7)])
    e = ref.elliptic()
    out.update(el_th1=th1, el_thJ=thJ, el_out1=np.asarray(e(th1)), el_outJ=np.asarray(e(thJ)),
               el_dG1=np.asarray(e(th1, dG=True)))
    np.random.seed(SEED)
    out["el_noisyJ"] = np.asarray(ref.elliptic(flag_noise=True)(thJ))      # (a single particle has no len(): blocks only)

    # ---- banana: one particle per call (a (2, J) block does not broadcast against the (2,) noise term) ----
    thb = np.vstack([rng.uniform(-2.0, 2.0, 5), rng.uniform(-3.0, 3.0, 5)])
    b = ref.banana()
    out.update(bn_th=thb, bn_out=np.stack([b(thb[:, j]) for j in range(thb.shape[1])], axis=1), bn_Gamma=b.Gamma)
    b2 = ref.banana(a=1.3, b=0.25, rho=0.5)
    out.update(bn2_prm=np.array([1.3, 0.25, 0.5]), bn2_out=np.stack([b2(thb[:, j]) for j in range(thb.shape[1])], axis=1),
               bn2_Gamma=b2.Gamma)
    np.random.seed(SEED)
    bn = ref.banana(flag_noise=True)
    out["bn_noisy"] = np.stack([bn(thb[:, j]) for j in range(thb.shape[1])], axis=1)
    # what the global RNG yields after a noise-FREE call: the reference draws its two normals either way
    np.random.seed(SEED)
    b(thb[:, 0])
    out["bn_rng_after_call"] = np.array(np.random.uniform())

    path = os.path.join(ROOT, "tests", "golden", "maps.npz")
    np.savez(path, **out)
    print("wrote %s (%d bytes, %d arrays)" % (path, os.path.getsize(path), len(out)))


if __name__ == "__main__":
    main()
