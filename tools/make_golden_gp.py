#!/usr/bin/env python3
"""Golden chains and predictions of the reference's Emulate stage and GP sampler (ces/emulate.py, ces/sample.py gp_mh
:17-119).

    python tools/make_golden_gp.py            # needs the reference checkout (CES_REFERENCE_ROOT)

Loads the REAL ces/emulate.py and ces/sample.py at run time with ``gpflow`` stubbed in ``sys.modules`` (``calibrate``
through oracle/_refload.py) and hands them this package's ``ces_amd.emulate.GPR`` models, rebuilt from the hyperparameters
stored here (GPflow cannot run here; parity with GPflow's own numbers is unpinned).  Writes only data -- the seeded inputs,
the hyperparameters and the reference's outputs -- to tests/golden/gp_mcmc.npz and tests/golden/gp_mcmc_manifest.json.
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
P, N, JT, STEPS = 2, 4, 30, 100

# name, kwargs of gp_mh (Gamma: None | 'diag' | 'dense'), enka.scaled, resume (steps of the first call)
CASES = [
    ("gamma_none", dict(), False, 0),
    ("gamma_diag", dict(Gamma="diag"), False, 0),
    ("gamma_dense", dict(Gamma="dense"), False, 0),
    ("compounded_diag", dict(Gamma="diag", noise_compounded=True), False, 0),
    ("compounded_dense", dict(Gamma="dense", noise_compounded=True), False, 0),
    ("pca", dict(Gamma="diag", pca=True), False, 0),
    ("pcn", dict(update="pCN", beta=0.4), False, 0),
    ("noscale", dict(delta=0.5, enka_scaling=False), False, 0),
    ("nonugget", dict(nugget=False, Gamma="diag", noise_compounded=True), False, 0),
    ("scaled", dict(delta=0.8), True, 0),
    ("resume", dict(delta=0.9), False, 60),
]
FAMILIES = ["RBF", "Matern12", "Matern32", "Matern52"]


def load_reference():
    pkg = types.ModuleType("refces")
    pkg.__path__ = []
    sys.modules["refces"] = pkg
    cal = _refload.load_reference_calibrate()
    sys.modules["refces.calibrate"] = cal
    pkg.calibrate = cal
    sys.modules.setdefault("gpflow", types.ModuleType("gpflow"))
    mods = {}
    for name in ("emulate", "sample"):
        path = os.path.join(_refload.REFERENCE_ROOT, "ces", name + ".py")
        with open(path) as fh:
            text = fh.read()
        mod = types.ModuleType("refces." + name)
        mod.__file__ = path
        mod.__package__ = "refces"
        sys.modules["refces." + name] = mod
        setattr(pkg, name, mod)
        exec(compile(_refload._retab(text), path, "exec"), mod.__dict__)
        mods[name] = mod
    return mods["emulate"], mods["sample"], cal


def problem(rng):
    """A mildly nonlinear map, its training ensemble and hand-set GP hyperparameters (one GP per output)."""
    A = rng.standard_normal((N, P))
    ustar = np.array([0.6, -0.3])
    Ustar = ustar[:, None] + 0.4 * rng.standard_normal((P, JT))
    Gstar = A @ Ustar + 0.2 * np.sin(2.0 * Ustar).sum(axis=0)
    hyp = dict(ls=np.array([[0.5 + 0.1 * i, 0.7 + 0.05 * i] for i in range(N)]),
               var=np.array([0.3 + 0.05 * i for i in range(N)]),
               lik=np.array([1e-3 * (1 + i) for i in range(N)]),
               mA=A.copy(), mb=0.05 * np.arange(N))
    y = A @ ustar + 0.2 * np.sin(2.0 * ustar).sum() + 0.05 * rng.standard_normal(N)
    return A, ustar, Ustar, Gstar, hyp, y


def build_gps(X, Gstar, hyp, family="Matern32", mean="Linear"):
    from ces_amd import emulate as em
    Kern = getattr(em, family)
    gps = []
    for i in range(Gstar.shape[0]):
        k = Kern(input_dim=X.shape[1], ARD=True, lengthscales=hyp["ls"][i], variance=hyp["var"][i])
        if mean == "Linear":
            mf = em.Linear(hyp["mA"][i].reshape(-1, 1), [hyp["mb"][i]])
        elif mean == "Constant":
            mf = em.Constant([hyp["mb"][i]])
        else:
            mf = None
        m = em.GPR(X, Gstar[i][:, None], k, mean_function=mf)
        m.likelihood.variance = hyp["lik"][i]
        gps.append(m)
    return gps


def make_enka(cal, Ustar, Gstar, scaled):
    enka = cal.enka(P, N, JT)
    enka.Ustar = Ustar
    enka.Gstar = Gstar
    if scaled:
        enka.scale = {"mean": Ustar.mean(axis=1)[:, None], "cov": 2.0 * np.linalg.cholesky(np.cov(Ustar))}
        enka.scaled = True
        X = np.linalg.solve(enka.scale["cov"], Ustar - enka.scale["mean"]).T
    else:
        X = Ustar.T
    return enka, X


def main():
    remu, rsmp, cal = load_reference()
    arrays, manifest = {}, dict(cases=[], predict=[], P=P, N=N, JT=JT, STEPS=STEPS)
    rng = np.random.default_rng(77)
    A, ustar, Ustar, Gstar, hyp, y = problem(rng)
    for key, val in dict(A=A, Ustar=Ustar, Gstar=Gstar, y=y, **{"hyp_" + k: v for k, v in hyp.items()}).items():
        arrays["prob_" + key] = val
    B = rng.standard_normal((N, N))
    gammas = dict(diag=np.diag(0.02 + 0.02 * rng.random(N)), dense=0.02 * (B @ B.T / N + 0.5 * np.eye(N)))
    arrays["prob_Gamma_diag"], arrays["prob_Gamma_dense"] = gammas["diag"], gammas["dense"]
    pca = dict(VD_k=np.eye(N) + 0.1 * rng.standard_normal((N, N)), mG=0.1 * rng.standard_normal((N, 1)))
    arrays["prob_VD_k"], arrays["prob_mG"] = pca["VD_k"], pca["mG"]
    mu, C = np.array([0.4, -0.2]), np.array([[1.0, 0.25], [0.25, 0.5]])
    arrays["prob_mu"], arrays["prob_Sigma"] = mu, C
    prior = stats.multivariate_normal(mean=mu, cov=C)

    for k, (name, kw, scaled, resume) in enumerate(CASES):
        seed = 2000 + k
        enka, X = make_enka(cal, Ustar, Gstar, scaled)
        enka.gpmodels = build_gps(X, Gstar, hyp)
        call = {kk: v for kk, v in kw.items() if kk not in ("Gamma", "pca")}
        if "Gamma" in kw:
            call["Gamma"] = gammas[kw["Gamma"]]
        if kw.get("pca"):
            call["pca_tools"] = pca
        mc = rsmp.MCMC()
        mc.mute_bar = True
        mc.y_obs = y
        np.random.seed(seed)
        if resume:
            mc.gp_mh(enka, resume, prior, **call)
            mc.gp_mh(enka, STEPS - resume, prior, **call)
        else:
            mc.gp_mh(enka, STEPS, prior, **call)
        tag = "mh_" + name + "_"
        arrays[tag + "samples"] = mc.samples
        arrays[tag + "accept"] = np.float64(mc.accept)
        manifest["cases"].append(dict(name=name, seed=seed, kwargs=kw, scaled=scaled, resume=resume))
        print("%-18s accept %.3f  samples %s" % (name, mc.accept, mc.samples.shape))

    # predict_gps for every kernel family and mean function, scaled and not, both nuggets
    Xq = np.vstack([Ustar[:, :3].T, ustar[None, :] + 0.5 * rng.standard_normal((5, P))])
    arrays["pred_X"] = Xq
    for fam in FAMILIES:
        for mean in ("Zero", "Constant", "Linear"):
            for scaled in (False, True):
                for nugget in (True, False):
                    enka, X = make_enka(cal, Ustar, Gstar, scaled)
                    enka.gpmodels = build_gps(X, Gstar, hyp, fam, mean)
                    m, v = remu.predict_gps(enka, Xq, nugget=nugget)
                    tag = "pred_%s_%s_%d_%d_" % (fam, mean, scaled, nugget)
                    arrays[tag + "mean"], arrays[tag + "var"] = m, v
                    manifest["predict"].append(dict(family=fam, mean=mean, scaled=scaled, nugget=nugget))
    enka, X = make_enka(cal, Ustar, Gstar, False)
    enka.gpmodels = build_gps(X, Gstar, hyp)
    m, v = remu.predict_gps(enka, Xq[:1], pca_tools=pca)
    arrays["pred_pca_mean"], arrays["pred_pca_var"] = m, v
    # scale_gppreds (outputs 2..6 log-normal) and scale_ensemble's AttributeError
    gm, gv = rng.standard_normal((8, 3)), 0.1 + rng.random((8, 3))
    Gm, Gs = rng.standard_normal(8), 0.5 + rng.random(8)
    sm, sv = remu.scale_gppreds(list(gm), list(gv), Gm, Gs)
    for key, val in dict(gm=gm, gv=gv, Gm=Gm, Gs=Gs, mean=sm, var=sv).items():
        arrays["sgp_" + key] = val
    enka = cal.enka(P, N, JT)
    enka.Ustar = Ustar
    try:
        remu.scale_ensemble(enka, factor=1.5)
        raise SystemExit("scale_ensemble did not raise")
    except AttributeError as exc:
        manifest["scale_ensemble_error"] = type(exc).__name__
    arrays["se_mean"], arrays["se_cov"] = enka.scale["mean"], enka.scale["cov"]
    np.savez_compressed(os.path.join(OUT, "gp_mcmc.npz"), **arrays)
    with open(os.path.join(OUT, "gp_mcmc_manifest.json"), "w") as fh:
        json.dump(manifest, fh, indent=1)


if __name__ == "__main__":
    main()
