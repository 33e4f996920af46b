"""Inputs shared by the device tests of the Emulate stage (test_gpu_gp.py, test_gpu_emulate_edges.py, test_gpu_gpfit.py,
test_gpu_engine_state.py): an enka with random GPs of given hyperparameters, and the training data of a fit problem."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_emulate_host import Enka, build_gps  # noqa: E402


def random_gps(rng, p, n, Jt, family, scaled=False, mean="Linear", lik=1e-4):
    U = rng.standard_normal((p, Jt))
    G = np.vstack([np.sin(U[i % p]) + 0.1 * i for i in range(n)])
    enka = Enka(p, n, U, G)
    X = U.T
    if scaled:
        enka.scale = {"mean": U.mean(axis=1)[:, None], "cov": 2.0 * np.linalg.cholesky(np.cov(U))}
        enka.scaled = True
        X = np.linalg.solve(enka.scale["cov"], U - enka.scale["mean"]).T
    hyp = dict(ls=0.6 + 0.5 * rng.random((n, p)), var=0.5 + rng.random(n), lik=lik * (1 + rng.random(n)),
               mA=0.3 * rng.standard_normal((n, p)), mb=rng.standard_normal(n))
    enka.gpmodels = build_gps(X, G, hyp, family, mean)
    return enka


def fit_problem(rng, Jt, p, n):
    X = rng.standard_normal((Jt, p))
    W = rng.standard_normal((p, n))
    Y = (np.sin(X @ W) + 0.2 * (X ** 2) @ np.abs(W) + 0.05 * rng.standard_normal((Jt, n))).T
    return X, Y
