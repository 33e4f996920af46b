"""The Sample stage's true-model sampler: a drop-in ``MCMC`` class for ``ces/sample.py`` (:12-202).

Same class name, constructor, attributes, method names, signatures and kwargs as the reference, so a caller switches
with ``from ces_amd import sample`` instead of ``from ces import sample``.  ``model_mh`` without build-only options is
the reference itself, restated in numpy on the host (one chain).  ``gp_mh`` needs a trained GP emulator (GPflow) and
raises ``ImportError`` -- the reference module fails the same way, earlier (its ``import gpflow``, :8).

Build-only extras of ``model_mh`` (not in the reference):
  kwarg ``chains=M``     run M independent chains on the GPU (libcesx, ``cesx_mh_*``): one chain per column of the
                         engine's (p, M) layout, the proposal an update launch, the forward map ``model.forward_device``,
                         the accept step ``mh_accept_kernel``.  Needs a model with ``forward_device`` (``ces_amd.utils.lineal``)
                         and a prior with ``.mean`` / ``.cov`` (a frozen ``scipy.stats.multivariate_normal``).
  kwarg ``start``        'mean' (default, the reference's start ``enka.Ustar.mean(axis=1)``) or 'ensemble' (chain j starts at
                         ``enka.Ustar[:, j]``, M <= J)
  ``self.engine_dtype``, ``self.noise`` ('numpy' | 'device'), ``self.seed``, ``self.device``, ``self.trace_stride``
                         mean what they mean on ``ces_amd.calibrate.sampling``.  With ``noise='numpy'`` every step draws
                         ``np.random.normal(0, 1, [p, M])`` and then ``np.random.uniform(size=M)``: for M = 1 the reference's
                         draws in the reference's order, so ``chains=1, start='mean'`` reproduces the reference chain.
  results                ``self.samples`` (p, n_kept) for M = 1 as in the reference, (p, n_kept, M) for M > 1 -- the first
                         state, every ``trace_stride``-th and the last; ``self.accept`` the overall rate;
                         ``self.accept_chains`` (M) the per-chain rates; ``self.samples_device`` the final states (device).
"""
import numpy as np

try:                                   # progress bars exactly where the reference has them
    from tqdm.autonotebook import tqdm
except Exception:                      # pragma: no cover - tqdm is optional plumbing
    def tqdm(it=None, **_kw):
        return it


class MCMC(object):
    """Metropolis-Hastings samplers of ces/sample.py (:12-202)."""

    def __init__(self):
        self.mute_bar = False
        # build-only (the device path of model_mh, chains=M)
        self.engine_dtype = "float64"
        self.noise = "numpy"
        self.seed = 1234
        self.device = 0
        self.trace_stride = 1

    def gp_mh(self, enka, n_mcmc, prior, delta=1., enka_scaling=True, **kwargs):
        """GP-based random-walk MH (ces/sample.py:17-119): needs a trained GPflow emulator (ces/emulate.py), which this
        package does not build."""
        raise ImportError("MCMC.gp_mh needs GPflow (a trained GP emulator, ces/emulate.py), which is not installed; "
                          "ces/sample.py fails the same way when it imports gpflow (:8)")

    def model_mh(self, model, n_mcmc, prior, enka, Gamma, delta=1., enka_scaling=True, **kwargs):
        """Random-walk / pCN Metropolis-Hastings on the true forward model (ces/sample.py:121-196).

        Without build-only kwargs this is the reference, restated on the host with its quirks:
          * RNG order per step: ``np.random.normal(0, 1, p)`` in the proposal (:199 / :202), then
            ``np.random.uniform()`` in the test (:188);
          * random walk: scales ``delta * chol(cov(enka.Ustar))`` (``enka_scaling``) or ``delta * I`` (:122-126);
          * pCN (``update='pCN'``): scales ``chol(prior.cov)`` whatever ``delta`` says (:127-129), the step
            ``sqrt(1 - beta**2) u + sqrt(beta) S xi`` with ``sqrt(beta)``, not ``beta`` (:202), and no prior term in phi
            (:143-145, :172-175);
          * any other ``update`` leaves the proposal unbound (:165-168): ``UnboundLocalError``;
          * a resume (``self.samples`` set) continues from ``samples[-1]`` while phi is still that of the start point
            ``enka.Ustar.mean(axis=1)``, and ``accept`` counts the new steps only (:131-163);
          * ``model.type == 'pde'`` runs ``enka.G_pde`` on ``[u, model.wt]`` at ``model.t`` (:133-137, :170-172).
        ``chains=M`` (build-only) runs M chains on the device (module docstring).  There a resume with
        ``noise='numpy'`` keeps the reference's phi of the start point; with ``noise='device'`` it is exact (phi of the
        resumed states, the step counter of the noise continues), so that two runs of n steps equal one of 2 n.
        """
        if kwargs.get("chains", None) is not None:
            return self._model_mh_device(model, n_mcmc, prior, enka, Gamma, delta, enka_scaling, kwargs)
        # RW needs the proposal distribution (:122-126)
        if enka_scaling:
            scales = delta * np.linalg.cholesky(np.cov(enka.Ustar).reshape(enka.p, enka.p))
        else:
            scales = delta * np.eye(enka.p)
        # pCN proposes according to the prior (:127-129)
        if kwargs.get("update", None) == "pCN":
            scales = np.linalg.cholesky(prior.cov)

        current = enka.Ustar.mean(axis=1)
        if model.type == "pde":
            w_mcmc = np.copy(model.wt)
            g = enka.G_pde(np.hstack([current.flatten(), w_mcmc]), model, model.t)
        else:
            g = enka.G(current.flatten(), model)

        yg = g[:enka.n_obs] - self.y_obs
        phi_current = (yg * np.linalg.solve(2 * Gamma, yg)).sum()
        if kwargs.get("update", None) != "pCN":           # pCN is prior invariant (:143-145)
            phi_current -= prior.logpdf(current.flatten())

        try:                                              # resume (:154-163)
            getattr(self, "samples")
            samples = list(self.samples.T)
            current = samples[-1]
            accept = 0
        except AttributeError:
            samples = []
            samples.append(current.flatten())
            accept = 0.

        for kk in tqdm(range(n_mcmc), desc="MCMC samples: ", disable=self.mute_bar):
            if kwargs.get("update", None) is None:
                proposal = self.random_walk(current, scales, enka.p)
            elif kwargs.get("update", None) == "pCN":
                proposal = self.pCN(current, scales, enka.p, beta=kwargs.get("beta", 0.5))

            if model.type == "pde":
                g_proposal = enka.G_pde(np.hstack([proposal.flatten(), w_mcmc]), model, model.t)
            else:
                g_proposal = enka.G(proposal.flatten(), model)

            yg = g_proposal[:enka.n_obs] - self.y_obs
            phi_proposal = (yg * np.linalg.solve(2 * Gamma, yg)).sum()
            if kwargs.get("update", None) != "pCN":
                phi_proposal -= prior.logpdf(proposal.flatten())

            if np.log(np.random.uniform()) < phi_current - phi_proposal:
                current = np.copy(proposal)
                phi_current = np.copy(phi_proposal)
                accept += 1.

            samples.append(current.flatten())

        self.samples = np.array(samples).T
        self.accept = accept / n_mcmc

    def random_walk(self, current, scales, n_dim):
        """ces/sample.py:198-199."""
        return current + np.matmul(scales, np.random.normal(0, 1, n_dim))

    def pCN(self, current, scales, n_dim, beta=0.5):
        """ces/sample.py:201-202 (sqrt(beta), as the reference has it)."""
        return np.sqrt(1 - beta**2) * current + np.sqrt(beta) * np.matmul(scales, np.random.normal(0, 1, n_dim))

    # -- build-only: M chains on the device ------------------------------------------------------------------------
    def _mh_engine(self, p, n, M):
        from . import engine as _engine
        key = (p, n, M, str(self.engine_dtype), int(self.device), int(self.seed))
        if getattr(self, "_mh_key", None) != key:
            self._mh_eng = _engine.Engine(p, n, M, dtype=str(self.engine_dtype), device=self.device, seed=self.seed)
            self._mh_key = key
        return self._mh_eng

    def _model_mh_device(self, model, n_mcmc, prior, enka, Gamma, delta, enka_scaling, kwargs):
        import torch
        from .utils import hook_takes_out
        M = kwargs["chains"]
        if isinstance(M, bool) or not isinstance(M, (int, np.integer)) or M < 1:
            raise ValueError("chains must be an integer >= 1, got %r" % (M,))
        M = int(M)
        if getattr(model, "type", None) == "pde" or not hasattr(model, "forward_device"):
            raise ValueError("chains=: the device path evaluates the forward map on the GPU through model.forward_device, "
                             "which %r does not offer ('pde' models keep their forward map on the host); run model_mh "
                             "without chains=" % (model,))
        if not (hasattr(prior, "mean") and hasattr(prior, "cov")):
            raise ValueError("chains=: the prior must expose .mean and .cov (a frozen scipy.stats.multivariate_normal does)")
        update = kwargs.get("update", None)
        if update not in (None, "pCN"):
            raise ValueError("chains=: unknown update %r (None or 'pCN')" % (update,))
        if self.noise not in ("numpy", "device"):
            raise ValueError("noise must be 'numpy' or 'device', got %r" % (self.noise,))
        p, n = enka.p, enka.n_obs
        # the scales exactly as the reference forms them (:122-129)
        if enka_scaling:
            scales = delta * np.linalg.cholesky(np.cov(enka.Ustar).reshape(p, p))
        else:
            scales = delta * np.eye(p)
        if update == "pCN":
            scales = np.linalg.cholesky(prior.cov)
        start = kwargs.get("start", "mean")
        if start == "mean":
            U0 = np.repeat(np.asarray(enka.Ustar, dtype=np.float64).mean(axis=1).reshape(p, 1), M, axis=1)
        elif start == "ensemble":
            if M > enka.Ustar.shape[1]:
                raise ValueError("start='ensemble' needs chains <= J = %d, got %d" % (enka.Ustar.shape[1], M))
            U0 = np.array(enka.Ustar[:, :M], dtype=np.float64)
        else:
            raise ValueError("start must be 'mean' or 'ensemble', got %r" % (start,))
        stride = max(1, int(self.trace_stride))
        mu = np.asarray(prior.mean, dtype=np.float64).reshape(p)
        cov = np.asarray(prior.cov, dtype=np.float64).reshape(p, p)

        eng = self._mh_engine(p, n, M)
        eng.set_problem(np.asarray(self.y_obs, dtype=np.float64).reshape(n), Gamma, mu, cov, mu)
        eng.mh_set_proposal(update, scales, kwargs.get("beta", 0.5))
        takes_out = hook_takes_out(model.forward_device)

        def fwd(u, out):
            if takes_out:
                return model.forward_device(eng, u, out=out)
            out.copy_(model.forward_device(eng, u))
            return out

        U = eng.to_device(U0, p, "mh_U").clone()
        G, P, GP = eng.empty(n), eng.empty(p), eng.empty(n)
        fwd(U, G)
        eng.mh_start(U, G)                                # phi of the start states (:131-152)
        resume = hasattr(self, "samples")
        if resume:
            prev = np.asarray(self.samples)
            if (M == 1 and prev.ndim != 2) or (M > 1 and (prev.ndim != 3 or prev.shape[2] != M)) or prev.shape[0] != p:
                raise ValueError("resume: self.samples %s does not hold %d chain(s) of dimension %d" % (prev.shape, M, p))
            last = prev[:, -1] if M == 1 else prev[:, -1, :]
            U = eng.to_device(np.ascontiguousarray(last.reshape(p, M)), p, "mh_U").clone()
            if self.noise == "device":                    # exact resume: phi of the resumed states
                fwd(U, G)
                eng.mh_start(U, G)
            base = int(getattr(self, "_mh_next_step", 0))
            kept = []
        else:
            prev = None
            base = 0
            kept = [U0.copy()]

        for k in tqdm(range(n_mcmc), desc="MCMC samples: ", disable=self.mute_bar):
            step = base + k
            xi_t = logu_t = None
            if self.noise == "numpy":
                xi = np.random.normal(0, 1, [p, M])       # :199 / :202
                logu = np.log(np.random.uniform(size=M))  # :188
                xi_t = eng.to_device(xi, p, "mh_xi")
                logu_t = torch.as_tensor(logu, dtype=torch.float64, device=eng.device)
            eng.mh_propose(step, U, xi=xi_t, out=P)
            fwd(P, GP)
            eng.mh_accept(step, U, P, GP, logu=logu_t)
            if (k + 1) % stride == 0 or k + 1 == n_mcmc:
                kept.append(eng.to_host(U))
        steps, rate, per = eng.mh_stats(per_chain=True)

        new = np.stack(kept, axis=1) if kept else np.zeros((p, 0, M))      # (p, n_new, M)
        if M == 1:
            new = new[:, :, 0]
        self.samples = new if prev is None else np.concatenate([prev, new], axis=1)
        self.accept = rate
        self.accept_chains = per.astype(np.float64) / max(1, n_mcmc)
        self.samples_device = U
        self._mh_next_step = base + n_mcmc
