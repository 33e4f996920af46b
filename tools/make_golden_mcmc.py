#!/usr/bin/env python3
"""Golden chains of the reference's true-model sampler (ces/sample.py MCMC.model_mh :121-196).

    python tools/make_golden_mcmc.py          # needs the reference checkout (CES_REFERENCE_ROOT)

Loads the REAL ces/sample.py at run time: ``gpflow`` and the package's ``emulate`` are stubbed in ``sys.modules``
(model_mh uses neither), ``calibrate`` comes through oracle/_refload.py.  Writes only data -- the seeded inputs and the
reference's ``samples`` / ``accept`` -- to tests/golden/mcmc.npz and tests/golden/mcmc_manifest.json.  No reference
source enters the repository.
"""
import json
import os
import sys
import types

import numpy as np
from scipy import stats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import _refload      # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
P, N, J, STEPS = 2, 10, 50, 200

# name, Gamma dense?, kwargs of model_mh, resume (steps of the first call; the second runs the rest)
CASES = [
    ("rw_diag", False, dict(delta=1.0, enka_scaling=True), 0),
    ("rw_dense_gamma", True, dict(delta=1.0, enka_scaling=True), 0),
    ("rw_noscale", False, dict(delta=0.3, enka_scaling=False), 0),
    ("pcn", False, dict(update="pCN", beta=0.3), 0),
    ("rw_resume", False, dict(delta=0.8, enka_scaling=True), 120),
]


def load_reference_sample():
    pkg = types.ModuleType("refces")
    pkg.__path__ = []
    sys.modules["refces"] = pkg
    cal = _refload.load_reference_calibrate()
    sys.modules["refces.calibrate"] = cal
    pkg.calibrate = cal
    emu = types.ModuleType("refces.emulate")
    sys.modules["refces.emulate"] = emu
    pkg.emulate = emu
    sys.modules.setdefault("gpflow", types.ModuleType("gpflow"))
    path = os.path.join(_refload.REFERENCE_ROOT, "ces", "sample.py")
    with open(path) as fh:
        text = fh.read()
    mod = types.ModuleType("refces.sample")
    mod.__file__ = path
    mod.__package__ = "refces"
    exec(compile(_refload._retab(text), path, "exec"), mod.__dict__)
    return mod, cal


def problem(rng, dense_gamma):
    A = rng.standard_normal((N, P))
    ustar = np.array([0.7, -0.4])
    if dense_gamma:
        B = rng.standard_normal((N, N))
        Gamma = 0.05 * (B @ B.T / N + 0.5 * np.eye(N))
    else:
        Gamma = np.diag(0.05 + 0.05 * rng.random(N))
    y = A @ ustar + rng.multivariate_normal(np.zeros(N), Gamma)
    mu = np.array([0.2, -0.1])
    C = np.array([[1.0, 0.3], [0.3, 0.6]])             # dense Sigma
    Ustar = ustar[:, None] + 0.3 * rng.standard_normal((P, J))
    return A, y, Gamma, mu, C, Ustar


def main():
    smod, cal = load_reference_sample()
    from oracle._refload import load_reference_utils
    ru = load_reference_utils()
    arrays, manifest = {}, []
    for k, (name, dense, kw, resume) in enumerate(CASES):
        seed = 1000 + k
        rng = np.random.default_rng(seed)
        A, y, Gamma, mu, C, Ustar = problem(rng, dense)
        model = ru.lineal(A)
        enka = cal.enka(P, N, J)
        enka.Ustar = Ustar
        prior = stats.multivariate_normal(mean=mu, cov=C)
        mc = smod.MCMC()
        mc.mute_bar = True
        mc.y_obs = y
        np.random.seed(seed)
        if resume:
            mc.model_mh(model, resume, prior, enka, Gamma, **kw)
            mc.model_mh(model, STEPS - resume, prior, enka, Gamma, **kw)
        else:
            mc.model_mh(model, STEPS, prior, enka, Gamma, **kw)
        tag = name + "_"
        for key, val in dict(A=A, y=y, Gamma=Gamma, mu=mu, Sigma=C, Ustar=Ustar, samples=mc.samples,
                             accept=np.float64(mc.accept)).items():
            arrays[tag + key] = val
        manifest.append(dict(name=name, seed=seed, kwargs=kw, resume=resume, steps=STEPS, p=P, n_obs=N, J=J))
        print("%-16s accept %.3f  samples %s" % (name, mc.accept, mc.samples.shape))
    np.savez_compressed(os.path.join(OUT, "mcmc.npz"), **arrays)
    with open(os.path.join(OUT, "mcmc_manifest.json"), "w") as fh:
        json.dump(manifest, fh, indent=1)


if __name__ == "__main__":
    main()
