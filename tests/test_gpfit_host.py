"""Training the emulators on device, the parts that need no GPU: ``fit_lockstep`` (the optimisers of all GPs in lockstep,
their likelihood evaluations batched) against sequential ``ScipyOptimizer`` fits, the C ABI's declarations, the register
budget of kernels_gpfit.hip on the ISA hipcc emits, and the argument check of ``train_gps(device=True)``."""
import os
import sys
import threading
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ces_amd import emulate as em          # noqa: E402

GPFIT_ENTRY_POINTS = ("cesx_gpfit_set", "cesx_gpfit_ntheta", "cesx_gpfit_eval", "cesx_gpfit_factors")
N_GP, J_T, P, MAXITER, BAD_GP, BAD_AT = 6, 120, 3, 200, 4, 3


class _FailingGPR(em.GPR):
    """A GPR whose ``fail_at``-th likelihood evaluation raises what a failed Cholesky raises."""
    fail_at, calls = 0, 0

    def log_marginal_likelihood_and_grad(self):
        self.calls += 1
        if self.calls == self.fail_at:
            raise np.linalg.LinAlgError("Matrix is not positive definite")
        return super().log_marginal_likelihood_and_grad()


def _problem(seed=3):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((J_T, P))
    W = rng.standard_normal((P, N_GP))
    Y = np.sin(X @ W) + 0.3 * (X ** 2) @ np.abs(W) + 0.05 * rng.standard_normal((J_T, N_GP))
    return X, Y.T


def _models(X, Y, cls_of=lambda i: em.GPR):
    return [cls_of(i)(X, Y[i][:, None], em.Matern32(input_dim=P, ARD=True), mean_function=em.Linear(np.ones((P, 1))))
            for i in range(N_GP)]


def _theta(m):
    pos, free = m._get()
    return np.concatenate([pos, free])


def test_fit_lockstep_is_bit_identical_to_sequential_fits():
    X, Y = _problem()
    seq = _models(X, Y, lambda i: _FailingGPR if i == BAD_GP else em.GPR)
    seq[BAD_GP].fail_at = BAD_AT
    seq_res = []
    for m in seq:
        seq_res.append(em.ScipyOptimizer().minimize(m, maxiter=MAXITER))

    par = _models(X, Y)
    seen = {i: 0 for i in range(N_GP)}
    batches, main = [], threading.get_ident()

    def evaluate(idx, thetas):
        assert threading.get_ident() == main                 # only the calling thread evaluates
        assert list(idx) == sorted(idx) and thetas.shape == (len(idx), 1 + P + 1 + P + 1)
        batches.append(len(idx))
        lml, grad, status = np.zeros(len(idx)), np.zeros(thetas.shape), np.zeros(len(idx), dtype=np.int32)
        for k, i in enumerate(idx):
            assert np.array_equal(thetas[k], _theta(par[i]))  # the model already holds the parameters it is asked at
            seen[i] += 1
            if i == BAD_GP and seen[i] == BAD_AT:
                status[k] = 2
                lml[k], grad[k] = np.nan, np.nan
            else:
                lml[k], grad[k] = par[i].log_marginal_likelihood_and_grad()
        return lml, grad, status

    opts = em.fit_lockstep(par, evaluate, maxiter=MAXITER)
    assert len(opts) == N_GP
    for i in range(N_GP):
        assert opts[i].result.nfev == seq_res[i].nfev == seen[i], i
        assert np.array_equal(opts[i].result.x, seq_res[i].x), i
        assert opts[i].result.fun == seq_res[i].fun, i
        assert np.array_equal(_theta(par[i]), _theta(seq[i])), i
    assert seen[BAD_GP] >= BAD_AT                              # the non-PD answer was really given
    assert len(batches) == max(r.nfev for r in seq_res)        # one batched call per lockstep round
    assert batches[0] == N_GP


def test_fit_lockstep_reraises_and_leaves_no_thread():
    X, Y = _problem(5)
    par = _models(X, Y)
    before = threading.active_count()
    calls = []

    def evaluate(idx, thetas):
        calls.append(len(idx))
        if len(calls) == 3:
            raise RuntimeError("evaluator failed")
        out = [par[i].log_marginal_likelihood_and_grad() for i in idx]
        return np.array([o[0] for o in out]), np.array([o[1] for o in out]), np.zeros(len(idx), dtype=np.int32)

    with pytest.raises(RuntimeError, match="evaluator failed"):
        em.fit_lockstep(par, evaluate, maxiter=50)
    assert len(calls) == 3
    assert threading.active_count() == before
    assert not [t for t in threading.enumerate() if t.name.startswith("fit_lockstep")]


def test_gpfit_abi_declared_exported_no_scratch():
    from ces_amd import engine
    with open(os.path.join(ROOT, "include", "cesx.h")) as fh:
        hdr = fh.read()
    for name in GPFIT_ENTRY_POINTS:
        assert name + "(" in hdr and name in engine.EXPORTS
    assert "#define CESX_ABI_VERSION %d" % engine.ABI_VERSION in hdr and engine.ABI_VERSION >= 2
    from ces_amd import build
    assert "kernels_gpfit.hip" in build.SOURCES
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_audit
    t = isa_audit.collect(["kernels_gpfit.hip"])
    rows = {k: v for k, v in t.items() if "gpfit_" in k}
    assert len(rows) == 8                                # prep, build, chol, kinv, tvec, alpha, grad, final
    for name, r in rows.items():
        assert r["ScratchSize [bytes/lane]"] == 0 and r["scratch_total"] == 0, name
        assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["spill_in_loop"] == 0, name
    mfma = {k: r for k, r in rows.items() if "gpfit_chol_kernel" in k or "gpfit_kinv_kernel" in k}
    assert len(mfma) == 2                                # factorisation + triangular inverse in one kernel; K^{-1} = W W^T
    for name, r in mfma.items():
        assert r["mfma_in_loop"] > 0, name


def test_train_gps_device_rejects_what_it_does_not_know_before_any_device_is_looked_for(monkeypatch):
    from ces_amd import engine

    def boom(*a, **k):
        raise AssertionError("the library was looked for")
    monkeypatch.setattr(engine, "load_library", boom)
    monkeypatch.setattr(engine, "Engine", boom)
    rng = np.random.default_rng(0)
    enka = types.SimpleNamespace(Ustar=rng.standard_normal((2, 20)), Gstar=rng.standard_normal((3, 20)), n_obs=3, p=2)

    class Periodic(em.Stationary):
        family = 9

    with pytest.raises(ValueError, match="on the host"):
        em.train_gps(enka, kernel=Periodic, device=True)
    with pytest.raises(ValueError, match="on the host"):
        em.train_gps(enka, kernel="Periodic", device=True)

    class Quadratic(object):
        def __call__(self, X):
            return np.zeros((np.asarray(X).shape[0], 1))

        def params(self):
            return []

    with pytest.raises(ValueError, match="on the host"):
        em.train_gps(enka, kernel="RBF", mean_function=Quadratic, device=True)
    with pytest.raises(TypeError, match="devcie_index"):
        em.train_gps(enka, kernel="RBF", device=True, devcie_index=1)
    assert not hasattr(enka, "gpmodels")
