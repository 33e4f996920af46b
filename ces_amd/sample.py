"""The Sample stage: a drop-in ``MCMC`` class for ``ces/sample.py`` (:12-202).

Same class name, constructor, attributes, method names, signatures and kwargs as the reference, so a caller switches
with ``from ces_amd import sample`` instead of ``from ces import sample``.  ``model_mh`` and ``gp_mh`` without build-only
options are the reference itself, restated in numpy on the host (one chain).  ``gp_mh`` samples the emulated posterior
of ``ces_amd.emulate`` (or of any objects with ``predict_y`` / ``predict_f`` passed as ``gpmodels``); with no emulator at
all it raises ``ImportError`` naming GPflow, as the reference module does without it.

Build-only extras of ``model_mh`` and ``gp_mh`` (not in the reference):
  kwarg ``chains=M``     run M independent chains on the GPU (libcesx, ``cesx_mh_*`` / ``cesx_gp_*``): one chain per column
                         of the engine's (p, M) layout, the proposal an update launch, then for model_mh the forward map
                         ``model.forward_device`` and ``mh_accept_kernel``, for gp_mh the batched GP prediction
                         ``gp_predict_kernel`` (fp64, MFMA) and ``gp_score_kernel``.  model_mh needs a model with
                         ``forward_device`` (``ces_amd.utils.lineal``) or, ``type == 'pde'``, ``forward_pde_device``
                         (``ces_amd.models`` lorenz63 / lorenz96 after ``set_solver(device=True)``: every chain integrates
                         from ``model.wt`` over ``model.t``; a proposal whose integration fails scores NaN and is
                         rejected, a start state that fails raises ``ValueError``); gp_mh needs this package's ``emulate.GPR`` models,
                         one per output, and keeps ``separable`` and ``noise_compounded`` with a dense Gamma and no
                         ``pca_tools`` on the host (ValueError).  Both need a prior with ``.mean`` / ``.cov`` (a frozen
                         ``scipy.stats.multivariate_normal``).
                         gp_mh with ``pca_tools=dict(VD_k=(n, k), mG=(n,) or (n, 1))`` and ``Gamma`` (required, dense or
                         diagonal) runs the PCA-decorrelated route on the device: k GPs, and per chain and state
                         ``Sigma = Gamma + VD_k diag(gvars) VD_k^T`` (ces/sample.py:52-53) built, factored and scored by
                         one wave (``gp_score_dense_kernel``, n <= 128), with 1/2 log det Sigma when
                         ``noise_compounded``.  ``pca_tools=dict(VD_k=np.eye(n), mG=np.zeros((n, 1)))`` gives the dense
                         compounded likelihood ``Gamma + diag(gvars)`` of :50-51 on the device.
  kwarg ``sigma_form``   with ``chains=``: 'dense' (default, the route above) or 'projected' -- needs ``pca_tools`` and
                         ``Gamma``; the same likelihood with Sigma projected to k x k (``emulate.project_sigma`` once on the
                         host, then ``gp_score_proj_kernel``: a k x k Cholesky per chain, several chains per wave), for any
                         n_obs and k <= 128.
  kwarg ``fused``        model_mh with ``chains=``: ``None`` (default) takes the fused chain kernel where the model's map has one
                         (``ces_amd.utils.elliptic`` and ``banana``: ``mh_run_map_kernel``, one chain per lane, up to
                         ``FUSED_STEPS_MAX`` Metropolis steps per launch -- proposal, map, phi and test in registers, fp64 for
                         either engine dtype; an fp32 engine's state is rounded at launch boundaries only) and the step path
                         (three launches per step) otherwise; ``False`` forces the step path; ``True`` on a model without a
                         fused kernel raises ``ValueError``.  Both paths draw the same noise and leave the same chains up to
                         the rounding of a different product order.
                         gp_mh with ``chains=``: ``True`` takes the fused chain kernel of the emulator (``gp_chain_kernel``,
                         ``cesx_gp_run``: one workgroup per 32 chains, per step the proposal, every GP's mean and variance on
                         one K* panel in LDS, phi and the test; the likelihoods Gamma, diag(gvars) and diag(Gamma) +
                         diag(gvars)); ``None`` (default, ``GP_FUSED_DEFAULT``) and ``False`` take the step path.  ``True``
                         with ``pca_tools`` (the dense and the projected Sigma stay on the step path) or ``separable``
                         raises ``ValueError``, and so does an emulator whose tile does not fit in LDS.  A launch runs at
                         most ``GP_FUSED_WORK`` of arithmetic.  ``self.fused_launches`` counts the fused launches of the last
                         call of either sampler (0: the step path).
  kwarg ``summary``      with ``chains=``: ``True`` sums the kept states on the device instead of copying them to the host
                         (``cesx_chain_summary_*``, kernels_chainsum.hip).  The draws are the states the trace would hold
                         but the start state -- after the call's steps s with ``s % trace_stride == 0`` -- that have
                         ``s > burn`` (kwarg ``burn``, steps, default 0; ``burn=`` without ``summary=True`` and fewer than 4
                         draws raise ``ValueError``).  ``self.summary`` is a dict of host fp64 values: ``n`` draws per chain
                         and ``chains``; ``mean`` (p,) and ``cov`` (p, p) pooled over all draws of all chains (ddof = 1);
                         ``within`` = W and ``between`` = B_m (p,), the mean variance and the variance of the means
                         (ddof = 1) of the 2 M half-chains (each chain's first and last n // 2 draws); ``rhat`` =
                         sqrt(((n_h - 1) / n_h W + B_m) / W) and ``ess`` = min(2 M n_h, 2 M var+ / B_m) with n_h = n // 2
                         (no rank normalisation, no autocorrelations: ``autocorr=`` has those).  The chains run exactly as without it;
                         ``self.samples`` gains only the start state (a fresh run) and the call's last state, so a resume
                         works, and a resumed call summarises its own steps.
  kwarg ``marginals``    with ``chains=`` and ``summary=True`` (``ValueError`` without): histograms of every parameter and of
                         chosen parameter pairs over exactly the draws the summary sums, counted on the device
                         (``cesx_chain_hist_*``, kernels_chainhist.hip).  ``None`` / ``False``: off; ``True``: the defaults; or a
                         dict with ``bins`` (64, 2 .. 256), ``bins2d`` (20 -- ``plots.find_levels``'s --, 2 .. 64), ``pairs``
                         (``None``, a list of (i, j), or 'all': every i < j, at most 64), ``range`` ((p, 2) rows [lo, hi]) and
                         ``width`` (6.0: without ``range``, row r spans mean_r -+ width std_r of ``enka.Ustar``, ddof = 1; a
                         zero spread raises ``ValueError``; with ``range``, ``width`` is not read); an unknown key raises ``ValueError``.  Edges are
                         ``np.linspace(lo, hi, bins + 1)``; the bin rule is ``numpy.histogram``'s, in fp64, and the counts
                         equal numpy's on the same draws bit for bit.  ``self.marginals`` is a dict of host arrays: ``n``,
                         ``chains``, ``edges`` (p, bins + 1), ``hist1d`` (p, bins) int64, ``below`` and ``above`` (p,) (draws
                         left of the range; right of it, and NaN), ``pairs`` (P, 2), ``edges2d`` (p, bins2d + 1), ``hist2d``
                         (P, bins2d, bins2d) int64 (row: the bin of the pair's first parameter) and ``outside2d`` (P,).
                         ``marginal_density`` and ``marginal_quantiles`` read it; ``plots.find_levels(H=hist2d[k])`` gives
                         the contour levels.  The chains, ``self.summary`` and ``self.samples`` are as without it.  A call
                         without ``marginals=`` removes ``self.marginals``: the attribute is always the last call's.
  kwarg ``autocorr``     with ``chains=`` and ``summary=True`` (``ValueError`` without): an effective sample size from the chains'
                         autocorrelations, over exactly the draws the summary sums, from lagged sums kept on the device
                         (``cesx_chain_acf_*``, kernels_chainacf.hip).  ``None`` / ``False``: off; ``True``: the defaults; an int:
                         ``lags``; or a dict with ``lags`` (31, 1 .. 64) and ``chains`` (``min(M, 1024)``: the first C chains are
                         followed); an unknown key, ``chains > M`` and fewer draws than ``lags + 2`` raise ``ValueError``.
                         ``self.autocorr`` (``finalise_autocorr``) is a dict of host fp64 values: ``n``, ``chains`` (C), ``lags``,
                         ``rho`` (p, lags + 1) the multi-chain autocorrelations 1 - (W - mean_j gamma_k) / var+, ``tau`` =
                         -1 + 2 sum of Geyer's initial monotone sequence of pairs rho_2t + rho_2t+1, ``ess`` = M n / tau (for
                         all M chains, from the C followed), ``truncated`` (p,) bool: no negative pair within the lags, so
                         ``ess`` is an over-estimate -- raise ``lags`` or ``trace_stride`` --, ``within`` = W and ``var_plus``.
                         A row in which no chain moved has ``ess = tau = nan``.  The chains, ``self.summary``,
                         ``self.marginals`` and ``self.samples`` are as without it; a call without ``autocorr=`` removes
                         ``self.autocorr``.  A host trace goes through ``autocorr_of_samples(samples, lags)``.
  kwarg ``update='langevin'``  gp_mh, on the host (one chain) and with ``chains=M``: a preconditioned Metropolis-adjusted
                         Langevin proposal from the closed-form gradients of the GPs (``emulate.GPR.predict_f_grad``; on the
                         device ``cesx_gp_predict_grad`` and ``cesx_gp_langevin_*``, kernels_gpgrad.hip).  With S the scales of
                         the random walk -- so ``delta`` is the Langevin step --, g(u) = S^T grad phi(u) and xi ~ N(0, I):
                         P = U + S (xi - g(U) / 2), accepted when
                         log u < phi(U) - phi(P) + |xi|^2 / 2 - |xi - (g(U) + g(P)) / 2|^2 / 2.  The draws per step are the random
                         walk's (xi, then u).  Likelihoods: Gamma (dense or diagonal), diag(gvars) and diag(Gamma) +
                         diag(gvars); and, with ``chains=M, sigma_form='projected'`` only, the Sigma of ``pca_tools``
                         (``cesx_gp_proj_langevin_*`` / ``cesx_gp_proj_hmc_*``: kernels_gpprojgrad.hip forms the coefficients of
                         grad m_t and grad v_t from the k x k factor per chain; ``MCMC.langevin_phi_grad_pca`` is the n-space
                         restatement).  ``fused=True``, ``pca_tools`` on the host or with ``sigma_form='dense'``, ``separable``,
                         emulators without gradients and Matern12 kernels raise ``ValueError``.  ``summary=``,
                         ``burn=``, ``marginals=``, ``start=``, ``noise=``, resume and ``trace_stride`` work as for the random walk.
                         model_mh takes it for a model with a Jacobian (``ces_amd.utils.elliptic`` and ``banana``:
                         ``model.jacobian`` on the host, ``model.jacobian_device`` -- ``cesx_map_jac`` -- with ``chains=M``): the
                         same step on the true posterior, phi with the prior term, grad phi = DG^T Gamma^{-1} (G - y) +
                         cov^{-1} (u - mean), the same scales, seed and draws, so its chains compare with the emulator's.
                         On the device the step path is ``cesx_mh_langevin_*`` (the emulator's lv_* kernels on G and DG) and
                         ``fused=True`` the fused kernel ``mh_langevin_map_kernel`` (``cesx_mh_langevin_run_map``: the chain and its
                         g in one lane's registers); ``fused=None`` is ``LANGEVIN_FUSED_DEFAULT``.  A resume always scores the
                         resumed states (phi and g).  The linear maps take it after ``model.enable_gradient()``
                         (``ces_amd.utils.lineal`` / ``lineal_log``, opt-in) at any p: their vector-Jacobian product
                         A^T Gamma^{-1} (G - y) (``lineal_log``: times exp(u)) is a GEMM, so with ``chains=M`` the step is
                         ``cesx_mh_langevin_lineal_*`` -- the gradient on the update kernels from images the engine forms
                         once (``model.langevin_device``), z = xi - g / 2 and the random walk's triangular launch for the
                         proposal, and one accept kernel (kernels_lvlin.hip) -- with no Jacobian image and no fused kernel
                         (``fused=True`` raises).  The Darcy models take it after ``model.enable_gradient()`` (``darcy.model`` /
                         ``model_trunc``, the resident solver): with ``chains=M`` a state costs ONE adjoint launch
                         (``model.gradient_device`` -- ``cesx_darcy_grad``: G, phi_d and d = d phi_d / du) and the step is
                         ``cesx_mh_langevin_*`` / ``cesx_mh_hmc_*`` under ``cesx_mh_grad_source(READY)``, which take d where the
                         closed-form maps hand over an (n_obs, p, M) Jacobian image (kernels_darcy_chain.hip: one wave per
                         chain); no fused kernel (``fused=True`` raises); a start state whose solve fails raises
                         ``ValueError``, a proposal or a leapfrog position whose solve fails is rejected.  A model without a
                         Jacobian (a plain ``lineal`` / ``lineal_log`` / Darcy model,
                         every 'pde' model) and ``flag_noise=True`` raise ``ValueError`` before an engine is created.
  kwarg ``update='hmc'``  model_mh and gp_mh, on the host (one chain) and with ``chains=M``: Hamiltonian Monte Carlo with kwarg
                         ``leapfrog=L`` (an integer in [1, 64], default 4) leapfrog steps per accept test, on the pieces of
                         ``update='langevin'`` -- its scales S (so ``delta`` is the leapfrog step; the mass matrix is
                         (S S^T)^-1), its g(u) = S^T grad phi(u), its phi with the prior term, its draws (xi, then u: ONE of each
                         per step whatever L is, so a run sees the noise of a Langevin run with the same seed):
                             r = xi - g(U) / 2;  Q = U;  L times  Q = Q + S r,  r = r - g(Q)  (r = r - g(Q) / 2 the last time);
                             accepted when  log u < phi(U) + |xi|^2 / 2 - phi(Q) - |r|^2 / 2.
                         At L = 1 this is the Langevin step term for term.  A NaN or an infinity anywhere in a trajectory
                         rejects.  With ``chains=M`` the proposal kind and the start are the Langevin step's
                         (``cesx_mh_langevin_start`` / ``cesx_gp_langevin_start``), the step path is ``cesx_mh_hmc_begin`` and per
                         leapfrog ``model.jacobian_device`` or ``cesx_gp_predict_grad`` and ``cesx_mh_hmc_leap`` / ``_accept``
                         (``cesx_gp_hmc_*`` on the emulator; kernels_hmc.hip), and for ``elliptic`` and ``banana`` ``fused=True``
                         the fused kernel ``mh_hmc_map_kernel`` (``cesx_mh_hmc_run_map``: the trajectory in one lane's registers,
                         at most ``HMC_GRADS_MAX`` gradient evaluations per launch, so a launch is ``HMC_GRADS_MAX // L`` steps at
                         the most); ``fused=None`` is ``LANGEVIN_FUSED_DEFAULT``; the emulator refuses ``fused=True``.
                         ``summary=``, ``burn=``, ``marginals=``, ``start=``, ``noise=``, sharded noise, resume (the resumed
                         states are scored through the Langevin start) and ``trace_stride`` work as for ``update='langevin'``.
                         The linear maps take it after ``model.enable_gradient(leapfrog=True)`` (opt-in) at any p: with
                         ``chains=M`` every position is update launches -- the gradient and the drift Q + S r of
                         ``cesx_mh_langevin_lineal_*`` around a momentum block of the engine dtype, ``cesx_mh_hmc_lineal_begin``
                         / ``_leap`` / ``_accept`` (kernels_hmclin.hip), the forward map once per position and phi at the last
                         one only --; L = 1 is ``update='langevin'`` bit for bit; no fused kernel (``fused=True`` raises).
                         It refuses what ``update='langevin'`` refuses, and the linear maps without that mark, with or without
                         ``enable_gradient()``; ``leapfrog=`` with any other ``update`` raises ``ValueError`` too.  No
                         trajectory-length adaptation; the step: ``adapt=``.
  kwarg ``adapt``        model_mh and gp_mh under ``update='langevin'`` and ``'hmc'``, on the host (one chain) and with ``chains=M``:
                         pooled step-size adaptation.  ``None`` / ``False``: off; ``True``: 100 steps; an int A: A steps; or a dict
                         with ``steps`` (100, 1 .. 65 536), ``target`` (0.574 under 'langevin', 0.651 under 'hmc'), ``gain`` (2)
                         and ``kappa`` (0.75); an unknown key raises ``ValueError``.  The first A of the call's ``n_mcmc`` steps
                         run at e S with one multiplier e shared by all chains (e_1 = 1; include/cesx.h, cesx_mh_adapt_*):
                             r = xi - (e / 2) g(U);  Q = U + e S r;  L - 1 times  r = r - e g(Q),  Q = Q + e S r;  r = r - (e / 2) g(Q);
                             d = phi(U) - phi(Q) + |xi|^2 / 2 - |r|^2 / 2;  accepted when log u < d;  alpha = min(1, exp d), 0 for a NaN;
                             log e_{t+1} = log e_t + (gain / sqrt(t)) (mean_j alpha_j - target);
                             log ebar_t = t^-kappa log e_{t+1} + (1 - t^-kappa) log ebar_{t-1}
                         ('langevin' is L = 1; the draws are the sampler's own, one xi and one u per step).  With ``chains=M``
                         they run on the step path whatever ``fused`` says, the mean and the recursion in ``ad_update_kernel``
                         behind every accept (kernels_adapt.hip): no synchronisation with the host inside the phase.  They are
                         kept in the trace like any other step.  Then ``delta' = float(delta) * ebar_A``, the scales are formed
                         again from ``delta'`` (a fresh run with ``delta=delta'`` sees the same bits), phi and g are re-scored
                         and the remaining ``n_mcmc - A`` steps run as without ``adapt=``, fused or not.  ``self.adapt`` is a
                         dict ``steps``, ``target``, ``multiplier``, ``delta`` (= delta'), ``accept_history`` and
                         ``multiplier_history`` (A,): the mean acceptance probability of every adaptation step and the e it ran
                         with; ``self.accept`` and ``self.accept_chains`` cover the steps at the frozen step.  A call without
                         ``adapt=`` removes ``self.adapt``.  ``ValueError`` before an engine is created: another ``update`` (the
                         random walk's and pCN's proposals are update launches), a linear map without the mark of
                         ``enable_gradient(leapfrog=True)`` (with it the phase runs on the ADAPT kernels of kernels_hmclin.hip,
                         armed behind the install and the start), ``A >= n_mcmc``, with ``chains=`` ``A % trace_stride != 0``
                         and ``summary=True`` with ``burn < A``.  Sharded chains are not pooled (``CESX_EUNSUPPORTED``).
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


def fused_chunks(n_mcmc, stride, steps_max, buffer_bytes, bytes_per_step, work_max=None, work_per_step=0):
    """The launches of a fused run of ``n_mcmc`` steps: ``(K_max, [K_0, K_1, ...])``, every launch ``K_max`` steps but the last.

    ``K_max`` is a multiple of ``stride`` -- so that a launch's own count of kept states continues the run's -- and as large
    as the caps allow: ``steps_max`` steps, ``buffer_bytes // bytes_per_step`` (one launch's noise and trace) and, with
    ``work_max``, ``work_max // work_per_step`` (the arithmetic of one launch).  A stride longer than every cap still makes
    one launch: ``K_max = stride``.  Pure: no engine, no device."""
    n_mcmc, stride = int(n_mcmc), max(1, int(stride))
    cap = min(int(steps_max), int(buffer_bytes) // max(1, int(bytes_per_step)))
    if work_max is not None and work_per_step > 0:
        cap = min(cap, int(work_max) // int(work_per_step))
    cap = max(1, cap)
    K_max = max(stride, cap // stride * stride)
    return K_max, [min(K_max, n_mcmc - k0) for k0 in range(0, n_mcmc, K_max)]


def _host_has_no_summary(kwargs):
    """``summary=``, ``burn=``, ``marginals=`` and ``autocorr=`` belong to the device paths of ``chains=M``."""
    for name in ("summary", "burn", "marginals", "autocorr"):
        if kwargs.get(name, None) is not None and not (name in ("marginals", "autocorr") and kwargs[name] is False):
            raise ValueError("%s=%r summarises the chains of chains=M on the device; the host path keeps every state in "
                             "self.samples" % (name, kwargs.get(name)))


def summary_draws(n_mcmc, stride, burn):
    """How many states of a call of ``n_mcmc`` steps ``summary=True`` summarises: the states after the steps s = 1 .. n_mcmc
    of the call with ``s % stride == 0`` (the ones the trace would hold; not the start state, not an off-stride last
    state) and ``s > burn``."""
    n_mcmc, stride, burn = int(n_mcmc), max(1, int(stride)), int(burn)
    return max(0, n_mcmc // stride - min(burn, n_mcmc) // stride)


def finalise_summary(raw, n_draws, chains):
    """The ``MCMC.summary`` dict from the raw sums of ``Engine.chain_summary_read`` (host numpy on p-sized arrays).

    ``raw``: ``c`` (p,) the pooled shift, ``s1`` (p,) = sum (x - c) and ``cc`` (p, p) = the lower triangle of
    sum (x - c)(x - c)^T over all N M draws, ``within`` = W and ``between`` = B_m of the 2 M half-chains of n = N // 2 draws.
    mean and cov pool all draws (ddof = 1); var+ = (n - 1) / n W + B_m, rhat = sqrt(var+ / W) and
    ess = min(2 M n, 2 M var+ / B_m): the split statistics without rank normalisation, and an effective sample size from
    the between-half-chain variance, not from autocorrelations."""
    N, M = int(n_draws), int(chains)
    c = np.asarray(raw["c"], dtype=np.float64)
    s1 = np.asarray(raw["s1"], dtype=np.float64)
    cc = np.tril(np.asarray(raw["cc"], dtype=np.float64))
    cc = cc + np.tril(cc, -1).T
    W = np.asarray(raw["within"], dtype=np.float64)
    B = np.asarray(raw["between"], dtype=np.float64)
    T, n = N * M, N // 2
    d = s1 / T
    with np.errstate(divide="ignore", invalid="ignore"):
        var_plus = (n - 1) / n * W + B
        rhat = np.sqrt(var_plus / W)
        ess = np.minimum(2.0 * M * n, 2.0 * M * var_plus / B)
    return dict(n=N, chains=M, mean=c + d, cov=(cc - T * np.outer(d, d)) / (T - 1), rhat=rhat, ess=ess, within=W, between=B)


AUTOCORR_KEYS = ("lags", "chains")
AUTOCORR_LAGS_DEFAULT, AUTOCORR_LAGS_MAX, AUTOCORR_CHAINS_DEFAULT = 31, 64, 1024      # CESX_CHAIN_ACF_LAGS_MAX


def autocorr_spec(autocorr, chains, summary, n_draws):
    """What ``autocorr=`` asks for: ``None`` (off: ``None`` / ``False``) or ``(lags, C)``.  ``True``: the defaults; an int:
    ``lags``; a dict: ``lags`` (31) and ``chains`` (``min(M, 1024)``).  ``ValueError`` for an unknown key, ``autocorr=`` without
    ``summary=True``, ``lags`` outside [1, 64], ``chains`` outside [1, M] and fewer than ``lags + 2`` draws.  Pure: no engine."""
    if autocorr is None or autocorr is False:
        return None
    if not summary:
        raise ValueError("autocorr=%r follows the draws summary=True sums; without summary=True every kept state is in "
                         "self.samples and autocorr_of_samples(self.samples, lags) reads them" % (autocorr,))
    if autocorr is True:
        autocorr = {}
    elif isinstance(autocorr, (int, np.integer)):
        autocorr = dict(lags=autocorr)
    if not isinstance(autocorr, dict):
        raise ValueError("autocorr must be None, False, True, an int (lags) or a dict with keys from %s, got %r" % (AUTOCORR_KEYS, autocorr))
    unknown = [k for k in autocorr if k not in AUTOCORR_KEYS]
    if unknown:
        raise ValueError("autocorr: unknown key(s) %s (known: %s)" % (sorted(map(str, unknown)), ", ".join(AUTOCORR_KEYS)))
    M = int(chains)
    L = autocorr.get("lags", AUTOCORR_LAGS_DEFAULT)
    C = autocorr.get("chains", min(M, AUTOCORR_CHAINS_DEFAULT))
    if isinstance(L, bool) or not isinstance(L, (int, np.integer)) or not 1 <= L <= AUTOCORR_LAGS_MAX:
        raise ValueError("autocorr: lags must be an integer in [1, %d], got %r" % (AUTOCORR_LAGS_MAX, L))
    if isinstance(C, bool) or not isinstance(C, (int, np.integer)) or not 1 <= C <= M:
        raise ValueError("autocorr: chains must be an integer in [1, %d] (the run's chains), got %r" % (M, C))
    if n_draws < max(4, int(L) + 2):
        raise ValueError("autocorr: %d draws per chain are fewer than lags + 2 = %d" % (n_draws, max(4, int(L) + 2)))
    return int(L), int(C)


def finalise_autocorr(raw, n, M_total, C, L):
    """The ``MCMC.autocorr`` dict from the raw sums of ``Engine.chain_acf_read`` (host numpy on (p, L + 1) arrays).

    ``raw``: ``gsum`` (p, L + 1) = sum over the C followed chains of G_k = sum_t (x_t - m)(x_{t+k} - m), m the chain's mean
    of its ``n`` draws; ``msum`` (p,) = sum (m_j - c) and ``m2sum`` (p,) = sum (m_j - c)^2 about any shift c.  With
    gamma_k = gsum_k / (C n): W = gsum_0 / (C (n - 1)), B / n = the ddof-1 variance of the chain means (0 for C = 1),
    var+ = (n - 1) / n W + B / n, rho_0 = 1, rho_k = 1 - (W - gamma_k) / var+; Geyer's pairs Pi_t = rho_2t + rho_2t+1 for
    t < (L + 1) // 2, cut at the first negative one and made monotone; tau = -1 + 2 sum Pi_t and ess = M_total n / tau: for
    all ``M_total`` chains of the run, from the C followed.  ``truncated``: no negative pair within the lags (ess is then an
    over-estimate).  A row with var+ = 0 -- no chain moved -- has ess = tau = nan."""
    n, M_total, C, L = int(n), int(M_total), int(C), int(L)
    g = np.asarray(raw["gsum"], dtype=np.float64).reshape(-1, L + 1)
    ms = np.asarray(raw["msum"], dtype=np.float64).reshape(-1)
    m2 = np.asarray(raw["m2sum"], dtype=np.float64).reshape(-1)
    p = g.shape[0]
    gam = g / (float(C) * n)
    W = g[:, 0] / (float(C) * (n - 1))
    Bn = np.maximum((m2 - ms * ms / C) / (C - 1), 0.0) if C > 1 else np.zeros(p)
    var_plus = (n - 1) / n * W + Bn
    rho = np.full((p, L + 1), np.nan)
    tau, truncated = np.full(p, np.nan), np.zeros(p, dtype=bool)
    for r in range(p):
        if not (np.isfinite(var_plus[r]) and var_plus[r] > 0.0):
            continue
        rho[r] = 1.0 - (W[r] - gam[r]) / var_plus[r]
        rho[r, 0] = 1.0
        total, last, cut = 0.0, np.inf, False
        for t in range((L + 1) // 2):
            pair = rho[r, 2 * t] + rho[r, 2 * t + 1]
            if pair < 0.0:
                cut = True
                break
            last = min(last, pair)
            total += last
        tau[r], truncated[r] = -1.0 + 2.0 * total, not cut
    with np.errstate(divide="ignore", invalid="ignore"):
        ess = M_total * n / tau
    return dict(n=n, chains=C, lags=L, rho=rho, tau=tau, ess=ess, truncated=truncated, within=W, var_plus=var_plus)


def autocorr_raw_of_samples(samples, lags):
    """The raw sums ``finalise_autocorr`` reads -- ``gsum`` (p, L + 1), ``msum``, ``m2sum`` (p,) --, and every chain's
    ``chain_gamma`` (L + 1, p, M) and ``chain_mean`` (p, M), from a host trace (p, n) or (p, n, M), centred sums in numpy."""
    x = np.asarray(samples, dtype=np.float64)
    if x.ndim == 2:
        x = x[:, :, None]
    if x.ndim != 3:
        raise ValueError("autocorr_of_samples: samples must have shape (p, n) or (p, n, M), got %s" % (x.shape,))
    p, n, M = x.shape
    L = lags
    if isinstance(L, bool) or not isinstance(L, (int, np.integer)) or L < 1:
        raise ValueError("autocorr_of_samples: lags must be an integer >= 1, got %r" % (lags,))
    if n < max(4, L + 2):
        raise ValueError("autocorr_of_samples: %d draws per chain are fewer than lags + 2 = %d" % (n, max(4, L + 2)))
    m = x.mean(axis=1)                                         # (p, M)
    z = x - m[:, None, :]
    gamma = np.stack([(z[:, :n - k] * z[:, k:]).sum(axis=1) for k in range(L + 1)])      # (L + 1, p, M)
    c = x[:, 0, :].mean(axis=1)
    dm = m - c[:, None]
    return dict(gsum=gamma.sum(axis=2).T.copy(), msum=dm.sum(axis=1), m2sum=(dm * dm).sum(axis=1), chain_gamma=gamma, chain_mean=m)


def autocorr_of_samples(samples, lags=AUTOCORR_LAGS_DEFAULT):
    """``MCMC.autocorr`` of a host trace ``samples`` (p, n) or (p, n, M): what ``autocorr=`` gives for the same draws, every
    chain followed (drop the start state and the burn-in first: every column counts as a draw)."""
    x = np.asarray(samples)
    M = 1 if x.ndim == 2 else x.shape[-1]
    raw = autocorr_raw_of_samples(x, lags)
    return finalise_autocorr(raw, x.shape[1], M, M, int(lags))


MARGINALS_KEYS = ("bins", "bins2d", "pairs", "range", "width")
MARGINALS_BINS_MAX, MARGINALS_BINS2D_MAX, MARGINALS_PAIRS_MAX = 256, 64, 64      # CESX_CHAIN_HIST_*_MAX


def marginals_spec(marginals, Ustar):
    """What ``marginals=`` asks for, as the arrays ``Engine.chain_hist_begin`` takes: ``None`` (off: ``None`` / ``False``) or a
    dict ``bins``, ``bins2d``, ``pairs`` (P, 2) int32, ``edges`` (p, bins + 1) and ``edges2d`` (p, bins2d + 1), fp64.

    ``True`` is ``{}``.  Keys: ``bins`` (64), ``bins2d`` (20, what ``plots.find_levels`` uses), ``pairs`` (None, a list of
    (i, j) with i != j, or 'all': every i < j), ``range`` ((p, 2) rows [lo, hi]; default row r of ``Ustar`` (p, J):
    mean_r -+ width std_r, ddof = 1) and ``width`` (6.0; not read with ``range``).  Row r's edges are ``np.linspace(lo_r, hi_r, bins + 1)``, computed
    here once: the device counts against these very bits.  Pure: no engine, no device; every refusal is a ValueError."""
    if marginals is None or marginals is False:
        return None
    if marginals is True:
        marginals = {}
    if not isinstance(marginals, dict):
        raise ValueError("marginals must be None, False, True or a dict with keys from %s, got %r" % (MARGINALS_KEYS, marginals))
    unknown = [k for k in marginals if k not in MARGINALS_KEYS]
    if unknown:
        raise ValueError("marginals: unknown key(s) %s (known: %s)" % (sorted(map(str, unknown)), ", ".join(MARGINALS_KEYS)))
    Ustar = np.asarray(Ustar, dtype=np.float64)
    p = Ustar.shape[0]
    sizes = {}
    for name, default, most in (("bins", 64, MARGINALS_BINS_MAX), ("bins2d", 20, MARGINALS_BINS2D_MAX)):
        v = marginals.get(name, default)
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 2 <= v <= most:
            raise ValueError("marginals: %s must be an integer in [2, %d], got %r" % (name, most, v))
        sizes[name] = int(v)
    pairs = marginals.get("pairs", None)
    if pairs is None:
        pairs = np.zeros((0, 2), dtype=np.int32)
    elif isinstance(pairs, str):
        if pairs != "all":
            raise ValueError("marginals: pairs must be None, a list of (i, j) or 'all', got %r" % (pairs,))
        if p * (p - 1) // 2 > MARGINALS_PAIRS_MAX:
            raise ValueError("marginals: pairs='all' is %d pairs at p = %d; at most %d are counted -- name the pairs"
                             % (p * (p - 1) // 2, p, MARGINALS_PAIRS_MAX))
        pairs = np.array([(i, j) for i in range(p) for j in range(i + 1, p)], dtype=np.int32).reshape(-1, 2)
    else:
        try:
            arr = np.asarray(pairs)
        except ValueError:                                # a ragged list
            arr = np.zeros(1)
        if arr.size == 0:
            arr = np.zeros((0, 2), dtype=np.int32)
        if arr.ndim != 2 or arr.shape[1] != 2 or not np.issubdtype(arr.dtype, np.integer):
            raise ValueError("marginals: pairs must be None, a list of (i, j) or 'all', got %r" % (pairs,))
        if len(arr) > MARGINALS_PAIRS_MAX:
            raise ValueError("marginals: %d pairs; at most %d are counted" % (len(arr), MARGINALS_PAIRS_MAX))
        if arr.size and (arr.min() < 0 or arr.max() >= p or np.any(arr[:, 0] == arr[:, 1])):
            raise ValueError("marginals: every pair (i, j) needs i != j and both in [0, %d), got %r" % (p, pairs))
        pairs = np.ascontiguousarray(arr, dtype=np.int32)
    rng = marginals.get("range", None)
    if rng is None:
        width = marginals.get("width", 6.0)
        if isinstance(width, bool) or not isinstance(width, (int, float, np.integer, np.floating)) or not (np.isfinite(width) and width > 0):
            raise ValueError("marginals: width must be a finite number > 0, got %r" % (width,))
        mean = Ustar.mean(axis=1)
        std = Ustar.std(axis=1, ddof=1) if Ustar.shape[1] > 1 else np.zeros(p)
        if not (np.all(np.isfinite(mean)) and np.all(np.isfinite(std)) and np.all(std > 0)):
            raise ValueError("marginals: the spread of enka.Ustar is zero or not finite in row(s) %s, so the default range "
                             "mean -+ width std is empty; pass range= (p, 2)"
                             % np.nonzero(~(np.isfinite(mean) & np.isfinite(std) & (std > 0)))[0].tolist())
        rng = np.stack([mean - float(width) * std, mean + float(width) * std], axis=1)
    else:
        rng = np.asarray(rng, dtype=np.float64)
        if rng.shape != (p, 2):
            raise ValueError("marginals: range must have shape (%d, 2), rows [lo, hi]; got %s" % (p, rng.shape))
    if not (np.all(np.isfinite(rng)) and np.all(rng[:, 0] < rng[:, 1])):
        raise ValueError("marginals: every row of the range needs finite lo < hi, got %r" % (rng.tolist(),))
    edges = np.stack([np.linspace(lo, hi, sizes["bins"] + 1) for lo, hi in rng])
    edges2d = np.stack([np.linspace(lo, hi, sizes["bins2d"] + 1) for lo, hi in rng])
    for e in (edges, edges2d):
        if not np.all(np.diff(e, axis=1) > 0):
            raise ValueError("marginals: a range is too narrow for its bins: the edges are not strictly increasing")
    return dict(bins=sizes["bins"], bins2d=sizes["bins2d"], pairs=pairs, edges=edges, edges2d=edges2d)


def marginal_density(marginals, row):
    """``(centres, density)`` of row ``row`` of ``MCMC.marginals``: the bin centres and count / (all draws x bin width).  The
    density integrates to the fraction of the draws inside the range (1 when ``below`` and ``above`` are 0)."""
    e = np.asarray(marginals["edges"][row], dtype=np.float64)
    h = np.asarray(marginals["hist1d"][row], dtype=np.float64)
    total = h.sum() + float(marginals["below"][row]) + float(marginals["above"][row])
    return 0.5 * (e[:-1] + e[1:]), h / (total * np.diff(e))


def marginal_quantiles(marginals, q):
    """The quantiles ``q`` (in [0, 1]) of every row from ``MCMC.marginals``: (p, len(q)).  The cumulative mass starts at
    ``below`` and ends short of 1 by ``above``; inside a bin it is linear (the draws taken as uniform over the bin), so the
    value is within one bin width of the sample quantile.  NaN where the quantile falls outside the range."""
    q = np.atleast_1d(np.asarray(q, dtype=np.float64))
    if np.any(~((q >= 0) & (q <= 1))):
        raise ValueError("marginal_quantiles: q must lie in [0, 1]")
    edges = np.asarray(marginals["edges"], dtype=np.float64)
    out = np.full((edges.shape[0], q.size), np.nan)
    for r in range(edges.shape[0]):
        h = np.asarray(marginals["hist1d"][r], dtype=np.float64)
        below, above = float(marginals["below"][r]), float(marginals["above"][r])
        total = h.sum() + below + above
        if total == 0:
            continue
        cum = below + np.concatenate([[0.0], np.cumsum(h)])        # the mass left of every edge
        nz = np.nonzero(h)[0]
        for i, t in enumerate(q * total):
            if t < cum[0] or t > cum[-1] or nz.size == 0:          # in the mass below or above the range
                continue
            k = int(np.searchsorted(cum, t, side="left"))          # the first edge with cum >= t: cum[k - 1] < t <= cum[k]
            if k == 0:                                             # t == below exactly: where the inside mass begins
                out[r, i] = edges[r, nz[0]]
            else:
                out[r, i] = edges[r, k - 1] + (t - cum[k - 1]) / (cum[k] - cum[k - 1]) * (edges[r, k] - edges[r, k - 1])
    return out


ADAPT_KEYS = ("steps", "target", "gain", "kappa")
ADAPT_STEPS_DEFAULT, ADAPT_STEPS_MAX = 100, 65536         # CESX_ADAPT_STEPS_MAX
ADAPT_TARGETS = {"langevin": 0.574, "hmc": 0.651}         # the optimal acceptance of MALA, and of HMC
ADAPT_GAIN, ADAPT_KAPPA = 2.0, 0.75


def adapt_spec(adapt, update):
    """What ``adapt=`` asks for: ``None`` (off: ``None`` / ``False``) or a dict ``steps``, ``target``, ``gain``, ``kappa``.
    ``True`` is 100 steps, an int A is A steps, a dict may hold the four keys (``target`` defaults to 0.574 under
    ``update='langevin'`` and 0.651 under ``'hmc'``, ``gain`` to 2, ``kappa`` to 0.75).  Pure; every refusal is a ValueError."""
    if adapt is None or adapt is False:
        return None
    if update not in ADAPT_TARGETS:
        raise ValueError("adapt=%r adapts the step of update='langevin' and 'hmc' (the multiplier scales the leapfrog step of "
                         "the gradient kernels); update=%r proposes through an update launch, whose scales are an image of "
                         "the proposal: tune delta by hand there" % (adapt, update))
    if adapt is True:
        adapt = {}
    elif isinstance(adapt, (int, np.integer)):
        adapt = dict(steps=adapt)
    if not isinstance(adapt, dict):
        raise ValueError("adapt must be None, False, True, an integer or a dict with keys from %s, got %r" % (ADAPT_KEYS, adapt))
    unknown = [k for k in adapt if k not in ADAPT_KEYS]
    if unknown:
        raise ValueError("adapt: unknown key(s) %s (known: %s)" % (sorted(map(str, unknown)), ", ".join(ADAPT_KEYS)))
    steps = adapt.get("steps", ADAPT_STEPS_DEFAULT)
    if isinstance(steps, bool) or not isinstance(steps, (int, np.integer)) or not 1 <= steps <= ADAPT_STEPS_MAX:
        raise ValueError("adapt: steps must be an integer in [1, %d], got %r" % (ADAPT_STEPS_MAX, steps))
    vals = {}
    for name, default, ok, what in (("target", ADAPT_TARGETS[update], lambda v: 0.0 < v < 1.0, "in (0, 1)"),
                                    ("gain", ADAPT_GAIN, lambda v: np.isfinite(v) and v > 0.0, "finite and > 0"),
                                    ("kappa", ADAPT_KAPPA, lambda v: 0.5 < v <= 1.0, "in (0.5, 1]")):
        v = adapt.get(name, default)
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not ok(v):
            raise ValueError("adapt: %s must be a number %s, got %r" % (name, what, v))
        vals[name] = float(v)
    return dict(steps=int(steps), **vals)


def adapt_recursion(log_e, log_ebar, t, abar, target, gain, kappa):
    """Step t >= 1 of the recursion of include/cesx.h (cesx_mh_adapt_*): ``(log e_{t+1}, log ebar_t)`` from ``log e_t``,
    ``log ebar_{t-1}`` and the mean acceptance probability ``abar`` of step t."""
    log_e = log_e + gain / np.sqrt(float(t)) * (abar - target)
    w = float(t) ** -kappa
    return log_e, w * log_e + (1.0 - w) * log_ebar


class MCMC(object):
    """Metropolis-Hastings samplers of ces/sample.py (:12-202)."""

    # build-only, model_mh(chains=, fused=): what fused=None resolves to for a model with a fused chain kernel (the measurement
    # behind it: NOTEBOOK.md, tools/map_mh_bench.py), the longest launch, and the bytes one launch's noise and trace may take
    FUSED_DEFAULT = True
    FUSED_STEPS_MAX = 4096
    FUSED_BUFFER_BYTES = 64 << 20
    # build-only, model_mh(chains=, update='langevin', fused=): what fused=None resolves to for elliptic and banana -- the path
    # that tools/map_langevin_bench.py measures faster at BOTH 1 024 and 65 536 chains on the elliptic problem (the step path
    # if the two sizes disagree).  Measured (NOTEBOOK.md): fused 5.3 us against 33.0 us per step at 1 024 chains, 13.5 us
    # against 43.8 us at 65 536, fp64 -- and on an fp64 engine both paths leave the same chains bit for bit.
    LANGEVIN_FUSED_DEFAULT = True
    # build-only, gp_mh(chains=, fused=): what fused=None resolves to (the step path: every call without fused= runs as it
    # did before the fused kernel existed; the measurement: NOTEBOOK.md, tools/gp_chain_bench.py), and the arithmetic one
    # launch may hold.  A fused gp step does real work -- per chain and GP the K* panel and its triangular product,
    # J_p (J_p / 2 + p + 8) multiply-adds -- so a launch is capped by K M n_gp J_p (J_p / 2 + p + 8) <= GP_FUSED_WORK as well.
    # The constant is 50 steps at shape E1 (65 536 chains, p = 8, 32 GPs, J_t = 512), where NOTEBOOK.md records 19 ms per
    # step: a launch of about 1 s on a card that others share, not the minute that FUSED_STEPS_MAX steps would take.
    GP_FUSED_DEFAULT = False
    GP_FUSED_WORK = 50 * 65536 * 32 * 512 * (512 // 2 + 8 + 8)

    def __init__(self):
        self.mute_bar = False
        # build-only (the device path of model_mh, chains=M)
        self.engine_dtype = "float64"
        self.noise = "numpy"
        self.seed = 1234
        self.device = 0
        self.trace_stride = 1

    def gp_mh(self, enka, n_mcmc, prior, delta=1., enka_scaling=True, **kwargs):
        """GP-based random-walk / pCN Metropolis-Hastings on the emulated posterior (ces/sample.py:17-119).

        Without build-only kwargs this is the reference, restated on the host with its quirks:
          * scales ``delta * chol(cov(enka.Ustar))`` (``enka_scaling``, no reshape) or ``delta * I`` (:23-26); pCN uses
            the SAME scales with ``sqrt(beta)`` (:72-73), and ``prior.logpdf`` is subtracted for RW and pCN alike (:57 / :96);
          * a resume (``self.samples`` set) takes ``samples[-1]`` BEFORE phi is computed: phi is that of the resumed
            state, unlike model_mh (:31-39);
          * Sigma (:48-55 / :87-94): Gamma None -> diag(gvars) plus 1/2 sum log gvars; ``noise_compounded`` without
            ``pca_tools`` -> Gamma + diag(gvars) plus 1/2 sum log eigvals(Sigma); with ``pca_tools`` -> Gamma + gvars;
            otherwise Gamma;
          * per step ``np.random.normal(0, 1, p)`` then ``np.random.uniform()``; an unknown ``update`` leaves the
            proposal unbound (``UnboundLocalError``).
        The emulator is ``kwargs['gpmodels']`` or ``enka.gpmodels`` (any objects with predict_y / predict_f); with
        neither the sampler raises ImportError naming GPflow, as the reference's own module does without it.
        ``chains=M`` (build-only) runs M chains on the device (module docstring).
        """
        if kwargs.get("gpmodels", None) is None and not hasattr(enka, "gpmodels"):
            raise ImportError("MCMC.gp_mh needs a trained GP emulator: pass gpmodels= or train enka.gpmodels with "
                              "ces_amd.emulate.train_gps (the reference builds it with GPflow, ces/emulate.py, which is "
                              "not installed; ces/sample.py fails when it imports gpflow, :8)")
        leapfrog = self._hmc_leapfrog(kwargs)             # build-only; refused before any engine is created
        if kwargs.get("adapt", None) not in (None, False) and kwargs.get("update", None) in ("langevin", "hmc"):
            if leapfrog is None:                          # (what update= refuses stays refused, with its own message)
                self._langevin_refusals(kwargs, prior)
            else:
                self._as_hmc(self._langevin_refusals, kwargs, prior)
        self._adapt_of(kwargs, n_mcmc)
        if kwargs.get("chains", None) is not None:
            return self._gp_mh_device(enka, n_mcmc, prior, delta, enka_scaling, kwargs)
        if kwargs.get("fused", None) is not None:
            raise ValueError("fused=%r chooses between the device paths of chains=M; the host path has one" % (kwargs.get("fused"),))
        if kwargs.get("sigma_form", None) is not None:
            raise ValueError("sigma_form=%r chooses between the device kernels of chains=M; the host path has one form"
                             % (kwargs.get("sigma_form"),))
        _host_has_no_summary(kwargs)
        from . import emulate
        if kwargs.get("update", None) in ("langevin", "hmc"):      # build-only
            return self._gp_mh_langevin_host(enka, n_mcmc, prior, delta, enka_scaling, kwargs)
        if enka_scaling:
            scales = delta * np.linalg.cholesky(np.cov(enka.Ustar))
        else:
            scales = delta * np.eye(enka.p)

        current = enka.Ustar.mean(axis=1)
        y = self.y_obs.reshape(-1, 1)

        try:                                              # resume (:31-39): before phi
            getattr(self, "samples")
            samples = list(self.samples.T)
            current = samples[-1]
            accept = 0
        except AttributeError:
            samples = []
            samples.append(current.flatten())
            accept = 0.

        def score(u):
            gmean, gvars = emulate.predict_gps(enka, u.reshape(1, -1),
                                               gpmodels=kwargs.get("gpmodels", None),
                                               nugget=kwargs.get("nugget", True),
                                               pca_tools=kwargs.get("pca_tools", None))
            yG = gmean - y
            if kwargs.get("Gamma", None) is None:
                Sigma = np.diag(gvars.flatten())
            elif kwargs.get("noise_compounded", False) and kwargs.get("pca_tools", None) is None:
                Sigma = kwargs.get("Gamma") + np.diag(gvars.flatten())
            elif kwargs.get("pca_tools", None) is not None:
                Sigma = kwargs.get("Gamma") + gvars
            else:
                Sigma = kwargs.get("Gamma")
            phi = (yG * np.linalg.solve(2 * Sigma, yG)).sum()
            phi -= prior.logpdf(u.flatten())
            if kwargs.get("Gamma", None) is None:
                phi += .5 * np.log(gvars).sum()
            elif kwargs.get("noise_compounded", False):
                phi += .5 * np.log(np.linalg.eigvals(Sigma)).sum()
            return phi

        phi_current = score(current)
        for k in tqdm(range(n_mcmc), desc="MCMC samples: ", disable=self.mute_bar):
            if kwargs.get("update", None) is None:
                proposal = self.random_walk(current, scales, enka.p)
            elif kwargs.get("update", None) == "pCN":
                proposal = self.pCN(current, scales, enka.p, beta=kwargs.get("beta", 0.5))
            phi_proposal = score(proposal)
            if np.log(np.random.uniform()) < phi_current - phi_proposal:
                current = np.copy(proposal)
                phi_current = np.copy(phi_proposal)
                accept += 1.
            samples.append(current)

        self.samples = np.array(samples).T
        self.accept = accept / n_mcmc

    HMC_LEAPFROG_DEFAULT, HMC_LEAPFROG_MAX = 4, 64        # CESX_HMC_LEAPFROG_MAX
    HMC_GRADS_MAX = 4096                                  # CESX_HMC_LAUNCH_GRADS_MAX: gradient evaluations per fused launch

    @staticmethod
    def _hmc_leapfrog(kwargs):
        """L of ``update='hmc'`` (kwarg ``leapfrog``, an integer in [1, 64], default 4), or None for every other update --
        which ``leapfrog=`` does not go with.  Every refusal is a ValueError."""
        L, update = kwargs.get("leapfrog", None), kwargs.get("update", None)
        if update != "hmc":
            if L is not None:
                raise ValueError("leapfrog=%r counts the leapfrog steps of update='hmc'; update=%r has none" % (L, update))
            return None
        L = MCMC.HMC_LEAPFROG_DEFAULT if L is None else L
        if isinstance(L, bool) or not isinstance(L, (int, np.integer)) or not 1 <= L <= MCMC.HMC_LEAPFROG_MAX:
            raise ValueError("update='hmc': leapfrog must be an integer in [1, %d], got %r" % (MCMC.HMC_LEAPFROG_MAX, L))
        return int(L)

    def _adapt_of(self, kwargs, n_mcmc, model=None):
        """The ``adapt_spec`` of a call, or None; what ``adapt=`` does not go with is a ValueError here, before an engine is
        created.  A call without ``adapt=`` removes ``self.adapt``: the attribute is always the last call's."""
        spec = adapt_spec(kwargs.get("adapt", None), kwargs.get("update", None))
        if spec is None:
            self.__dict__.pop("adapt", None)
            return None
        A = spec["steps"]
        if (model is not None and not getattr(model, "leapfrog_device", False)
                and (getattr(model, "model_name", None) in ("lineal", "lineal_log") or hasattr(model, "langevin_device"))):
            raise ValueError("adapt=: %r is a linear map, whose Langevin step is the GEMM form of kernels_lvlin.hip (the "
                             "gradient on the update kernels); the multiplier lives in the leapfrog kernels: the follow-up of "
                             "kernels_hmclin.hip, which enable_gradient(leapfrog=True) opts into -- call that, tune delta by "
                             "hand, or adapt on elliptic / banana or on the emulator (gp_mh)" % (model,))
        if A >= int(n_mcmc):
            raise ValueError("adapt=: the first %d of the call's n_mcmc steps adapt, and n_mcmc = %d leaves none at the step "
                             "found" % (A, int(n_mcmc)))
        if kwargs.get("chains", None) is not None:
            stride = max(1, int(self.trace_stride))
            if A % stride:
                raise ValueError("adapt=: %d adaptation steps at trace_stride %d: the state after the last of them must be a "
                                 "kept one, and fused launches start on a stride boundary; make steps a multiple of the stride"
                                 % (A, stride))
            burn = kwargs.get("burn", None)
            if kwargs.get("summary", None) is True and (isinstance(burn, bool) or not isinstance(burn, (int, np.integer)) or burn < A):
                raise ValueError("adapt=: summary=True with burn=%r would summarise states drawn while the step still moved; "
                                 "pass burn >= %d (the adaptation steps)" % (burn, A))
        return spec

    def _adapt_host(self, spec, score, scales, current, leapfrog, samples):
        """The adaptation phase on the host, one chain (M = 1 of include/cesx.h, cesx_mh_adapt_*): ``spec['steps']`` steps from
        ``current`` at e S, e following the recursion; every state is appended to ``samples``.  ``score`` is the sampler's own
        (phi, g = S^T grad phi).  Returns (the last state, the multiplier ebar_A, the history (A, 2) of (e_t, alpha_t))."""
        L = 1 if leapfrog is None else leapfrog
        p = scales.shape[0]
        phi, g = score(current)
        log_e = log_ebar = 0.0
        hist = np.zeros((spec["steps"], 2))
        for t in range(1, spec["steps"] + 1):
            e = float(np.exp(log_e))
            xi = np.random.normal(0, 1, p)
            with np.errstate(invalid="ignore", over="ignore"):
                r = xi - 0.5 * e * g
                q = current + e * np.matmul(scales, r)
                for l in range(1, L + 1):
                    phi_q, g_q = score(q)
                    if l < L:
                        r = r - e * g_q
                        if not np.isfinite(phi_q):
                            r = r * np.nan
                        q = q + e * np.matmul(scales, r)
                    else:
                        r = r - 0.5 * e * g_q
                d = phi - phi_q + (0.5 * (xi * xi).sum() - 0.5 * (r * r).sum())
                alpha = 1.0 if d >= 0 else float(np.exp(d)) if d < 0 else 0.0
            if np.log(np.random.uniform()) < d:
                current, phi, g = np.copy(q), phi_q, g_q
            samples.append(current.flatten())
            hist[t - 1] = e, alpha
            log_e, log_ebar = adapt_recursion(log_e, log_ebar, t, alpha, spec["target"], spec["gain"], spec["kappa"])
        return current, float(np.exp(log_ebar)), hist

    def _adapt_result(self, spec, multiplier, delta, hist):
        self.adapt = dict(steps=spec["steps"], target=spec["target"], multiplier=float(multiplier), delta=float(delta),
                          accept_history=np.array(hist[:, 1]), multiplier_history=np.array(hist[:, 0]))

    @staticmethod
    def _as_hmc(refusals, *args):
        """``update='hmc'`` refuses what ``update='langevin'`` refuses, by the same function: its ValueError under hmc's name."""
        try:
            refusals(*args)
        except ValueError as exc:
            raise ValueError(str(exc).replace("update='langevin'", "update='hmc'"))

    @staticmethod
    def hmc_trajectory(score, scales, current, g_current, xi, leapfrog):
        """The leapfrog trajectory of one HMC step from ``current`` (p,) with g = S^T grad phi there: r = xi - g / 2, then
        ``leapfrog`` times q = q + S r, (phi, g) = ``score(q)``, r = r - g (r = r - g / 2 at the last).  A non-finite phi in
        mid-trajectory poisons r, as the kernels do.  Returns (q, phi(q), g(q), r)."""
        r = xi - 0.5 * g_current
        q = current
        for l in range(1, leapfrog + 1):
            q = q + np.matmul(scales, r)
            phi_q, g_q = score(q)
            if l < leapfrog:
                r = r - g_q
                if not np.isfinite(phi_q):
                    r = r * np.nan
            else:
                r = r - 0.5 * g_q
        return q, phi_q, g_q, r

    @staticmethod
    def _langevin_refusals(kwargs, prior):
        """What ``gp_mh(update='langevin')`` cannot do, host and device alike: every refusal is a ValueError with the reason."""
        projected = False
        if kwargs.get("pca_tools", None) is not None:     # differentiated on the device alone, in the projected form
            projected = kwargs.get("chains", None) is not None and kwargs.get("sigma_form", None) == "projected"
            if not projected:
                raise ValueError("update='langevin': pca_tools has a gradient path only as chains=M, sigma_form='projected' (the "
                                 "k x k projected Sigma is differentiated on the device); the host path and sigma_form='dense' "
                                 "have none: pass chains=M, sigma_form='projected', or run the random walk (update=None) with "
                                 "pca_tools")
        if kwargs.get("separable", False):
            raise ValueError("update='langevin': separable predicts one point at a time and has no gradient path")
        if not (hasattr(prior, "mean") and hasattr(prior, "cov")):
            raise ValueError("update='langevin': the prior must expose .mean and .cov (its gradient is cov^{-1} (u - mean))")
        Gamma = kwargs.get("Gamma", None)
        if Gamma is not None and kwargs.get("noise_compounded", False) and not projected:
            G = np.asarray(Gamma, dtype=np.float64)
            if np.any(G != np.diag(np.diag(G))):
                raise ValueError("update='langevin': noise_compounded with a dense Gamma has no gradient path (Gamma + "
                                 "diag(gvars) would be factored per state); pass a diagonal Gamma")

    @staticmethod
    def langevin_phi_grad(mean, var, dmean, dvar, u, y, Gamma, compounded, prior_mean, prior_cov):
        """phi (up to the prior's constant) and grad phi at the states ``u`` (N, p) from the GP rows ``mean``, ``var`` (n, N)
        and their gradients ``dmean``, ``dvar`` (n, N, p): the formulas of include/cesx.h (cesx_gp_langevin_*) in numpy,
        vectorised over the states.  ``Gamma`` None: Sigma = diag(var); ``compounded``: diag(Gamma) + diag(var); else Gamma."""
        d = mean - np.asarray(y, dtype=np.float64).reshape(-1, 1)                   # (n, N)
        if Gamma is not None and not compounded:
            a = np.linalg.solve(np.asarray(Gamma, dtype=np.float64), d)
            phi = 0.5 * (d * a).sum(axis=0)
            grad = np.einsum("in,inq->nq", a, dmean)
        else:
            v = var if Gamma is None else var + np.diag(np.asarray(Gamma, dtype=np.float64)).reshape(-1, 1)
            with np.errstate(divide="ignore", invalid="ignore"):
                phi = 0.5 * (d * d / v + np.log(v)).sum(axis=0)
                a, b = d / v, 0.5 * (1.0 / v - d * d / (v * v))
            grad = np.einsum("in,inq->nq", a, dmean) + np.einsum("in,inq->nq", b, dvar)
        w = np.linalg.solve(np.asarray(prior_cov, dtype=np.float64), (u - np.asarray(prior_mean, dtype=np.float64).reshape(1, -1)).T)
        phi = phi + 0.5 * ((u - np.asarray(prior_mean, dtype=np.float64).reshape(1, -1)).T * w).sum(axis=0)
        return phi, grad + w.T

    @staticmethod
    def langevin_phi_grad_pca(mean, var, dmean, dvar, u, y, Gamma, VD_k, mG, logdet, prior_mean, prior_cov):
        """phi (up to the prior's constant) and grad phi at the states ``u`` (N, p) under ``pca_tools``: the k GP rows ``mean``,
        ``var`` (k, N) and their gradients ``dmean``, ``dvar`` (k, N, p), B = ``VD_k`` (n, k), d = B m + mG - y and
        Sigma_j = Gamma + B diag(v_j) B^T.  The literal n-space form in numpy, vectorised over the states -- ``solve`` with
        Sigma_j, e = B^T Sigma^{-1} d, h = diag(B^T Sigma^{-1} B) --
            phi = 1/2 d^T Sigma^{-1} d [+ 1/2 log det Sigma]                      (``logdet``: noise_compounded)
            grad phi = sum_t (e_t grad m_t + 1/2 ([logdet] h_t - e_t^2) grad v_t) + prior_cov^{-1} (u - prior_mean):
        the restatement the device's projected form (include/cesx.h, cesx_gp_proj_langevin_*) is held to.  A state whose
        Sigma is not positive definite has phi = NaN."""
        B = np.asarray(VD_k, dtype=np.float64)
        n, k = B.shape
        Gam = np.asarray(Gamma, dtype=np.float64).reshape(n, n)
        mean, var = np.asarray(mean, dtype=np.float64), np.asarray(var, dtype=np.float64)
        N = mean.shape[1]
        d = B @ mean + np.asarray(mG, dtype=np.float64).reshape(n, 1) - np.asarray(y, dtype=np.float64).reshape(n, 1)      # (n, N)
        Sig = Gam[None] + np.einsum("it,tj,lt->jil", B, var, B)                      # (N, n, n)
        rhs = np.concatenate([d.T[:, :, None], np.broadcast_to(B, (N, n, k))], axis=2)
        with np.errstate(invalid="ignore", divide="ignore"):
            ev = np.linalg.eigvalsh(Sig)
            sol = np.linalg.solve(Sig, rhs)                                          # Sigma^{-1} [d | B]
            e = np.einsum("it,ji->tj", B, sol[:, :, 0])                              # (k, N)
            phi = 0.5 * (d.T * sol[:, :, 0]).sum(axis=1)
            b = -0.5 * e * e
            if logdet:
                h = np.einsum("it,jit->tj", B, sol[:, :, 1:])
                phi = phi + 0.5 * np.log(ev).sum(axis=1)
                b = 0.5 * (h - e * e)
            phi = np.where(ev[:, 0] > 0.0, phi, np.nan)
        grad = np.einsum("tn,tnq->nq", e, dmean) + np.einsum("tn,tnq->nq", b, dvar)
        du = (u - np.asarray(prior_mean, dtype=np.float64).reshape(1, -1)).T
        w = np.linalg.solve(np.asarray(prior_cov, dtype=np.float64), du)
        return phi + 0.5 * (du * w).sum(axis=0), grad + w.T

    @staticmethod
    def langevin_correction(xi, g_current, g_proposal):
        """log q(U | P) - log q(P | U) of the proposal P = U + S (xi - g(U) / 2), the short way: no S^{-1}, because
        S^{-1} (P - U + S g(U) / 2) = xi by construction.  The last axis is the parameter axis."""
        back = xi - 0.5 * (g_current + g_proposal)
        return 0.5 * (xi * xi).sum(axis=-1) - 0.5 * (back * back).sum(axis=-1)

    def _gp_mh_langevin_host(self, enka, n_mcmc, prior, delta, enka_scaling, kwargs):
        """``gp_mh(update='langevin')`` on the host, one chain (module docstring): the restatement the device is held to.
        The scales, the start, the resume (phi and g of the resumed state) and the draws per step are the random walk's."""
        from . import emulate
        leapfrog = self._hmc_leapfrog(kwargs)             # None: the Langevin step
        if leapfrog is None:
            self._langevin_refusals(kwargs, prior)
        else:
            self._as_hmc(self._langevin_refusals, kwargs, prior)
        p = enka.p
        scales = delta * np.linalg.cholesky(np.cov(enka.Ustar).reshape(p, p)) if enka_scaling else delta * np.eye(p)
        Gamma, compounded = kwargs.get("Gamma", None), bool(kwargs.get("noise_compounded", False))

        def score(u):
            try:
                rows = emulate.predict_gps(enka, u.reshape(1, -1), gpmodels=kwargs.get("gpmodels", None),
                                           nugget=kwargs.get("nugget", True), grad=True)
            except ValueError as exc:
                raise ValueError("update=%r: %s" % (kwargs.get("update"), exc))
            phi, grad = self.langevin_phi_grad(*rows, u.reshape(1, -1), self.y_obs, Gamma, compounded, prior.mean, prior.cov)
            return phi[0], scales.T @ grad[0]

        current = enka.Ustar.mean(axis=1)
        if hasattr(self, "samples"):                      # resume: before phi, as gp_mh's random walk
            samples = list(self.samples.T)
            current = samples[-1]
        else:
            samples = [current.flatten()]
        accept = 0.
        adapt = self._adapt_of(kwargs, n_mcmc)
        if adapt:                                         # the first steps at e S; then the scales re-formed from delta', phi and g re-scored
            current, mult, hist = self._adapt_host(adapt, score, scales, current, leapfrog, samples)
            delta = float(delta) * mult
            scales = delta * np.linalg.cholesky(np.cov(enka.Ustar).reshape(p, p)) if enka_scaling else delta * np.eye(p)
            self._adapt_result(adapt, mult, delta, hist)
            n_mcmc = n_mcmc - adapt["steps"]
        phi_current, g_current = score(current)
        for k in tqdm(range(n_mcmc), desc="MCMC samples: ", disable=self.mute_bar):
            xi = np.random.normal(0, 1, p)
            if leapfrog is None:
                proposal = current + np.matmul(scales, xi - 0.5 * g_current)
                phi_proposal, g_proposal = score(proposal)
                corr = self.langevin_correction(xi, g_current, g_proposal)
            else:                                         # update='hmc': the kinetic energies stand where the correction stands
                proposal, phi_proposal, g_proposal, r = self.hmc_trajectory(score, scales, current, g_current, xi, leapfrog)
                corr = 0.5 * (xi * xi).sum() - 0.5 * (r * r).sum()
            if np.log(np.random.uniform()) < phi_current - phi_proposal + corr:
                current, phi_current, g_current = np.copy(proposal), phi_proposal, g_proposal
                accept += 1.
            samples.append(current)
        self.samples = np.array(samples).T
        self.accept = accept / n_mcmc

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
        ``update='langevin'`` (build-only): the Metropolis-adjusted Langevin step for a model that offers its gradient --
        ``elliptic`` and ``banana`` (``jacobian`` / ``jacobian_device``), ``lineal`` and ``lineal_log`` after
        ``enable_gradient()`` (``jacobian`` / ``langevin_device``: the adjoint launches of cesx_mh_langevin_lineal_*, at any
        p), and ``darcy.model`` / ``model_trunc`` after ``enable_gradient()`` (on the host ``jacobian``: one sparse LU and
        n_obs adjoint solves per state; with ``chains=M`` ``gradient_device``: one adjoint launch per position, and the
        Langevin / leapfrog entry points under ``cesx_mh_grad_source(READY)`` -- ``update='hmc'``, ``leapfrog=``, ``adapt=``,
        ``summary=`` and the rest as for ``elliptic``, no fused kernel); module docstring.
        """
        leapfrog = self._hmc_leapfrog(kwargs)             # build-only; refused before any engine is created
        if kwargs.get("update", None) == "langevin":
            self._model_langevin_refusals(model, prior, kwargs.get("chains", None) is not None)
        if leapfrog is not None:
            self._model_hmc_refusals(model, prior, kwargs.get("chains", None) is not None)
        adapt = self._adapt_of(kwargs, n_mcmc, model)
        if kwargs.get("chains", None) is not None:
            return self._model_mh_device(model, n_mcmc, prior, enka, Gamma, delta, enka_scaling, kwargs)
        if kwargs.get("fused", None) is not None:
            raise ValueError("fused=%r chooses between the device paths of chains=M; the host path has one" % (kwargs.get("fused"),))
        _host_has_no_summary(kwargs)
        if kwargs.get("update", None) in ("langevin", "hmc"):
            return self._model_mh_langevin_host(model, n_mcmc, prior, enka, Gamma, delta, enka_scaling, leapfrog=leapfrog, adapt=adapt)
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

    @staticmethod
    def _model_langevin_refusals(model, prior, device):
        """What ``model_mh(update='langevin')`` cannot do, host and device alike: every refusal is a ValueError with the reason."""
        need = "jacobian_device" if device else "jacobian"
        # (langevin_device: the adjoint launches of the linear maps; gradient_device: the adjoint launch of the Darcy models)
        has = hasattr(model, need) or (device and (hasattr(model, "langevin_device") or hasattr(model, "gradient_device")))
        if getattr(model, "type", None) == "pde" or not hasattr(model, "jacobian") or not has:
            raise ValueError("update='langevin' needs the gradient of phi, and %r offers no Jacobian (model.%s; "
                             "ces_amd.utils.elliptic and banana do, lineal and lineal_log after enable_gradient(): their "
                             "gradient is an A^T product, the Darcy models after enable_gradient(): chains=M takes their "
                             "adjoint launch, model.gradient_device); the Lorenz models have no adjoint; "
                             "gp_mh(update='langevin') differentiates the emulator instead" % (model, need))
        if getattr(model, "flag_noise", False):
            raise ValueError("update='langevin': a noisy map (flag_noise=True) has no gradient of phi")
        if not (hasattr(prior, "mean") and hasattr(prior, "cov")):
            raise ValueError("update='langevin': the prior must expose .mean and .cov (its gradient is cov^{-1} (u - mean))")

    @staticmethod
    def _model_hmc_refusals(model, prior, device):
        """What ``model_mh(update='hmc')`` cannot do: the linear maps without the mark of ``enable_gradient(leapfrog=True)``
        (their gradient is a GEMM on the update kernels; the GEMM-form leapfrog of kernels_hmclin.hip is opt-in), then everything
        ``update='langevin'`` refuses."""
        if (not getattr(model, "leapfrog_device", False)
                and (getattr(model, "model_name", None) in ("lineal", "lineal_log") or hasattr(model, "langevin_device"))):
            raise ValueError("update='hmc': %r is a linear map, with or without enable_gradient(); its gradient is an A^T "
                             "product on the update kernels and the GEMM-form leapfrog (the follow-up of the Langevin step, "
                             "kernels_hmclin.hip) is opt-in -- call enable_gradient(leapfrog=True), run update='langevin' after "
                             "enable_gradient(), or update='hmc' on elliptic / banana" % (model,))
        MCMC._as_hmc(MCMC._model_langevin_refusals, model, prior, device)

    def _model_mh_langevin_host(self, model, n_mcmc, prior, enka, Gamma, delta, enka_scaling, leapfrog=None, adapt=None):
        """``model_mh(update='langevin')`` on the host, one chain: the restatement the device is held to.  The scales and
        the start are the random walk's, phi has the prior term, g = S^T grad phi with
        grad phi = DG^T Gamma^{-1} (G - y) + cov^{-1} (u - mean) from ``model.jacobian``; the proposal
        ``u + S (xi - g / 2)``, the test with ``langevin_correction``, and the draws per step in the order of the host
        ``gp_mh(update='langevin')``: ``np.random.normal(0, 1, p)``, then ``np.random.uniform()``.  A resume scores the
        resumed state (phi and g)."""
        p, n = enka.p, enka.n_obs
        scales = delta * np.linalg.cholesky(np.cov(enka.Ustar).reshape(p, p)) if enka_scaling else delta * np.eye(p)
        Gamma = np.asarray(Gamma, dtype=np.float64).reshape(n, n)
        mean = np.asarray(prior.mean, dtype=np.float64).reshape(p)
        cov = np.asarray(prior.cov, dtype=np.float64).reshape(p, p)
        y = np.asarray(self.y_obs, dtype=np.float64).reshape(n)

        def score(u):
            yg = np.asarray(enka.G(u.flatten(), model), dtype=np.float64)[:n] - y
            a = np.linalg.solve(Gamma, yg)
            w = np.linalg.solve(cov, u.flatten() - mean)
            DG = np.asarray(model.jacobian(u.flatten()), dtype=np.float64).reshape(n, p)
            phi = 0.5 * (yg * a).sum() + 0.5 * ((u.flatten() - mean) * w).sum()
            return phi, scales.T @ (DG.T @ a + w)

        current = enka.Ustar.mean(axis=1)
        if hasattr(self, "samples"):
            samples = list(self.samples.T)
            current = samples[-1]
        else:
            samples = [current.flatten()]
        accept = 0.
        if adapt:                                         # the first steps at e S; then the scales re-formed from delta', phi and g re-scored
            current, mult, hist = self._adapt_host(adapt, score, scales, current, leapfrog, samples)
            delta = float(delta) * mult
            scales = delta * np.linalg.cholesky(np.cov(enka.Ustar).reshape(p, p)) if enka_scaling else delta * np.eye(p)
            self._adapt_result(adapt, mult, delta, hist)
            n_mcmc = n_mcmc - adapt["steps"]
        phi_current, g_current = score(current)
        for k in tqdm(range(n_mcmc), desc="MCMC samples: ", disable=self.mute_bar):
            xi = np.random.normal(0, 1, p)
            if leapfrog is None:
                proposal = current + np.matmul(scales, xi - 0.5 * g_current)
                phi_proposal, g_proposal = score(proposal)
                corr = self.langevin_correction(xi, g_current, g_proposal)
            else:                                         # update='hmc' (``leapfrog`` positions per test): module docstring
                proposal, phi_proposal, g_proposal, r = self.hmc_trajectory(score, scales, current, g_current, xi, leapfrog)
                corr = 0.5 * (xi * xi).sum() - 0.5 * (r * r).sum()
            if np.log(np.random.uniform()) < phi_current - phi_proposal + corr:
                current, phi_current, g_current = np.copy(proposal), phi_proposal, g_proposal
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

    def _mh_device(self, enka, n_mcmc, prior, kwargs, Gamma, scales_of, bind, resume_keeps_start_phi, fused=False,
                   fused_work=0, langevin=False, fused_steps_max=None, adapt=None, bind_adapt=None, delta=1.,
                   arm_after_start=False):
        """M = kwargs['chains'] chains on the engine: what ``model_mh(chains=)`` and ``gp_mh(chains=)`` have in common.

        Gamma                    the data covariance handed to ``set_problem``
        scales_of(update)        the proposal scales S (p, p), formed once ``prior`` and ``update`` have been checked
        bind(eng, M)             runs after ``mh_set_proposal``; returns ``score_start(U)`` (phi of the states U into the
                                 engine, counters cleared), ``score_accept(step, U, P, logu)`` (phi of P, the test, U := P
                                 where it passes) and ``run_steps(step, K, U, stride, trace, xi, logu)`` (K steps in one
                                 launch: ``eng.mh_run_map`` for a map, ``eng.gp_run`` for the emulator; None where the
                                 sampler has no fused kernel) and, optionally, a fourth hook ``propose(step, U, xi, P)`` that
                                 stands in for ``eng.mh_propose`` on the step path (the Langevin proposal reads the chains' g)
        langevin                 the sampler takes ``update='langevin'`` and ``'hmc'`` (gp_mh; model_mh for a model with a Jacobian)
        fused_steps_max          the longest fused launch in steps (None: ``FUSED_STEPS_MAX``; update='hmc': ``HMC_GRADS_MAX``
                                 over the leapfrog count).  ``run_steps`` may return the launches it made (None: one)
        resume_keeps_start_phi   the reference's model_mh scores the START point before it looks for ``self.samples`` and
                                 keeps that phi for the resumed states (ces/sample.py:131-163); its gp_mh scores the resumed
                                 states (:31-39).  True: the first, for ``noise='numpy'`` (``noise='device'`` re-scores the
                                 resumed states either way: the exact resume of model_mh's docstring)
        fused                    the steps run through ``run_steps`` (K Metropolis steps per launch) instead of propose /
                                 ``score_accept``
        fused_work               the arithmetic of one fused step of all chains, in the units of ``GP_FUSED_WORK`` (0: a launch
                                 is capped by ``FUSED_STEPS_MAX`` and ``FUSED_BUFFER_BYTES`` alone)
        adapt, bind_adapt, delta ``adapt_spec``'s dict (``_adapt_of`` has refused what it does not go with): the call's first
                                 ``adapt['steps']`` steps run on the step path of an armed engine (``eng.mh_adapt_set``) through
                                 the hooks of ``bind_adapt(eng, M)`` -- the leapfrog hooks, L = 1 for update='langevin' --;
                                 then ``eng.mh_adapt_read`` (the one synchronisation), the scales re-formed by
                                 ``scales_of(update, delta * multiplier)``, ``mh_set_proposal``, ``bind`` and ``score_start``
                                 again, and the remaining steps as without it.  ``self.adapt`` holds what was found
        arm_after_start          when the engine is armed: False -- before ``bind_adapt`` and the start, as the models with a
                                 Jacobian image and the emulator take it --; True -- behind them: the linear maps' install
                                 (cesx_mh_langevin_lineal_set) and start (cesx_mh_langevin_lineal_start) refuse an armed handle
        ``self.fused_launches`` is the number of fused launches of the call, 0 on the step path.
        ``kwargs['summary'] = True`` (with ``kwargs['burn']`` steps left out) keeps the kept states on the device and sums
        them there (``eng.chain_summary_*``): ``self.summary`` (``finalise_summary``) instead of a trace in ``self.samples``,
        which gains the start state of a fresh run and the call's last state only.  The chains run as without it.
        ``kwargs['marginals']`` (``marginals_spec``; needs ``summary=True``) counts the same draws into histograms on the device
        (``eng.chain_hist_*``): ``self.marginals``.  The chains and ``self.summary`` are as without it.
        ``kwargs['autocorr']`` (``autocorr_spec``; needs ``summary=True``) keeps the lagged sums of the same draws on the device
        (``eng.chain_acf_*``): ``self.autocorr`` (``finalise_autocorr``).  Everything else is as without it.
        """
        import torch
        M = kwargs["chains"]
        if isinstance(M, bool) or not isinstance(M, (int, np.integer)) or M < 1:
            raise ValueError("chains must be an integer >= 1, got %r" % (M,))
        M = int(M)
        if not (hasattr(prior, "mean") and hasattr(prior, "cov")):
            raise ValueError("chains=: the prior must expose .mean and .cov (a frozen scipy.stats.multivariate_normal does)")
        update = kwargs.get("update", None)
        if update in ("langevin", "hmc") and not langevin:
            raise ValueError("chains=: update='langevin' / 'hmc' needs the gradient of phi, and this sampler has no Jacobian on the "
                             "device; gp_mh(chains=, update='langevin') differentiates the emulator")
        if update not in (None, "pCN", "langevin", "hmc"):
            raise ValueError("chains=: unknown update %r (None, 'pCN', 'langevin' or 'hmc')" % (update,))
        if self.noise not in ("numpy", "device"):
            raise ValueError("noise must be 'numpy' or 'device', got %r" % (self.noise,))
        stride = max(1, int(self.trace_stride))
        summary, burn = kwargs.get("summary", None), kwargs.get("burn", None)
        if summary not in (None, False, True):
            raise ValueError("summary must be None, False or True, got %r" % (summary,))
        summary = bool(summary)
        if burn is not None and not summary:
            raise ValueError("burn=%r counts the steps summary=True leaves out; without summary=True every kept state is in "
                             "self.samples" % (burn,))
        if summary:
            burn = 0 if burn is None else burn
            if isinstance(burn, bool) or not isinstance(burn, (int, np.integer)) or burn < 0:
                raise ValueError("burn must be an integer >= 0 (steps), got %r" % (burn,))
            burn = int(burn)
            n_draws = summary_draws(n_mcmc, stride, burn)
            if n_draws < 4:
                raise ValueError("summary=True: %d steps at trace_stride %d with burn=%d leave %d draws per chain; the split "
                                 "statistics need 4 (two half-chains of two)" % (n_mcmc, stride, burn, n_draws))
        marg = kwargs.get("marginals", None)
        if marg is not None and marg is not False and not summary:
            raise ValueError("marginals=%r counts the draws summary=True sums; without summary=True every kept state is in "
                             "self.samples and numpy.histogram counts them" % (marg,))
        marg = marginals_spec(marg, enka.Ustar)
        acf = autocorr_spec(kwargs.get("autocorr", None), M, summary, n_draws if summary else 0)
        p, n = enka.p, enka.n_obs
        scales = scales_of(update)
        start = kwargs.get("start", "mean")
        if start == "mean":
            U0 = np.repeat(np.asarray(enka.Ustar, dtype=np.float64).mean(axis=1).reshape(p, 1), M, axis=1)
        elif start == "ensemble":
            if M > enka.Ustar.shape[1]:
                raise ValueError("start='ensemble' needs chains <= J = %d, got %d" % (enka.Ustar.shape[1], M))
            U0 = np.array(enka.Ustar[:, :M], dtype=np.float64)
        else:
            raise ValueError("start must be 'mean' or 'ensemble', got %r" % (start,))
        mu = np.asarray(prior.mean, dtype=np.float64).reshape(p)
        cov = np.asarray(prior.cov, dtype=np.float64).reshape(p, p)

        eng = self._mh_engine(p, n, M)
        eng.set_problem(np.asarray(self.y_obs, dtype=np.float64).reshape(n), Gamma, mu, cov, mu)
        eng.mh_set_proposal(update, scales, kwargs.get("beta", 0.5))
        if adapt and not arm_after_start:                 # armed: the leapfrog launches run at e S until the next mh_set_proposal
            eng.mh_adapt_set(adapt["steps"], adapt["target"], adapt["gain"], adapt["kappa"])
        score_start, score_accept, run_steps, propose = (tuple((bind_adapt if adapt else bind)(eng, M)) + (None,))[:4]
        P = eng.empty(p)
        self.fused_launches = 0

        resume = hasattr(self, "samples")
        prev, base, kept = None, 0, [U0.copy()]
        if not resume or resume_keeps_start_phi:
            U = eng.to_device(U0, p, "mh_U").clone()
            score_start(U)
        if resume:
            prev = np.asarray(self.samples)
            if (M == 1 and prev.ndim != 2) or (M > 1 and (prev.ndim != 3 or prev.shape[2] != M)) or prev.shape[0] != p:
                raise ValueError("resume: self.samples %s does not hold %d chain(s) of dimension %d" % (prev.shape, M, p))
            last = prev[:, -1] if M == 1 else prev[:, -1, :]
            U = eng.to_device(np.ascontiguousarray(last.reshape(p, M)), p, "mh_U").clone()
            if not resume_keeps_start_phi or self.noise == "device":
                score_start(U)
            base, kept = int(getattr(self, "_mh_next_step", 0)), []
        if adapt and arm_after_start:                     # (the install and every start above ran unarmed)
            eng.mh_adapt_set(adapt["steps"], adapt["target"], adapt["gain"], adapt["kappa"])
        if summary:                                       # the draws stay on the device: cesx_chain_summary_*
            eng.chain_summary_begin(n_draws)
        if marg:                                          # and are counted there: cesx_chain_hist_*, the same slices
            eng.chain_hist_begin(marg["edges"], marg["edges2d"], marg["pairs"])
        if acf:                                           # and their lagged sums are kept there: cesx_chain_acf_*, the same slices
            eng.chain_acf_begin(n_draws, acf[0], acf[1])

        def run_fused(k_first, n_steps):
            # launches of at most K_max steps (cesx_mh_run_map / cesx_gp_run; fused_chunks): K_max a multiple of the stride --
            # so that a launch's own count of kept states continues the run's -- and small enough that one launch's noise and
            # trace stay under the budget and, for the emulator, its arithmetic under GP_FUSED_WORK.
            # The trace buffer is allocated once per run; each launch's trace crosses to the host once.
            esz = eng.np_dtype.itemsize
            per_step = -(-M * p * esz // stride) + (M * (p * esz + 8) if self.noise == "numpy" else 0)     # trace; xi and log u
            K_max, chunks = fused_chunks(n_steps, stride, fused_steps_max or self.FUSED_STEPS_MAX, self.FUSED_BUFFER_BYTES, per_step,
                                         self.GP_FUSED_WORK if fused_work else None, fused_work)
            trace = torch.empty((min(K_max, n_steps) // stride, p, M), dtype=eng.torch_dtype, device=eng.device)
            for i, K in enumerate(tqdm(chunks, desc="MCMC samples: ", disable=self.mute_bar)):
                k0 = k_first + i * K_max
                xi_t = logu_t = None
                if self.noise == "numpy":                 # the step loop's draws in the step loop's order, stacked
                    xi, logu = np.empty((K, p, M)), np.empty((K, M))
                    for k in range(K):
                        xi[k] = np.random.normal(0, 1, [p, M])
                        logu[k] = np.log(np.random.uniform(size=M))
                    xi_t = torch.as_tensor(xi, device=eng.device).to(eng.torch_dtype).contiguous()
                    logu_t = torch.as_tensor(logu, dtype=torch.float64, device=eng.device)
                tr = trace[:K // stride]
                self.fused_launches += run_steps(base + k0, K, U, stride, tr, xi_t, logu_t) or 1
                if summary:                               # the launch's states after the steps s = k0 + stride (t + 1) > burn
                    t0 = max(0, burn // stride - k0 // stride)
                    if t0 < K // stride:
                        eng.chain_summary_add(tr[t0:])
                        if marg:
                            eng.chain_hist_add(tr[t0:])
                        if acf:
                            eng.chain_acf_add(tr[t0:])
                elif K // stride:
                    kept.extend(tr.cpu().numpy().astype(np.float64))
            if (summary or n_mcmc % stride) and n_mcmc > 0:   # the run's last state, where the trace does not hold it
                kept.append(eng.to_host(U))

        def run_step_path(k_first, n_steps):
            for k in tqdm(range(k_first, k_first + n_steps), desc="MCMC samples: ", disable=self.mute_bar):
                step = base + k
                xi_t = logu_t = None
                if self.noise == "numpy":                     # the reference's draws in the reference's order
                    xi = np.random.normal(0, 1, [p, M])       # :199 / :202
                    logu = np.log(np.random.uniform(size=M))  # :188 / :98
                    xi_t = eng.to_device(xi, p, "mh_xi")
                    logu_t = torch.as_tensor(logu, dtype=torch.float64, device=eng.device)
                if propose is None:
                    eng.mh_propose(step, U, xi=xi_t, out=P)
                else:
                    propose(step, U, xi_t, P)
                score_accept(step, U, P, logu_t)
                if summary:
                    if (k + 1) % stride == 0 and k + 1 > burn:
                        eng.chain_summary_add(U)
                        if marg:
                            eng.chain_hist_add(U)
                        if acf:
                            eng.chain_acf_add(U)
                    if k + 1 == n_mcmc:
                        kept.append(eng.to_host(U))
                elif (k + 1) % stride == 0 or k + 1 == n_mcmc:
                    kept.append(eng.to_host(U))

        first = 0
        if adapt:
            # the adaptation steps on the step path whatever ``fused`` says, kept in the trace like any other step; then the
            # join: read (the one synchronisation), delta' = delta * multiplier, the scales re-formed from delta' by
            # scales_of's own expression (a fresh run with delta=delta' sees the same bits), the proposal, the hooks, phi and g
            first = adapt["steps"]
            run_step_path(0, first)
            found = eng.mh_adapt_read()
            delta = float(delta) * found["multiplier"]
            self._adapt_result(adapt, found["multiplier"], delta, found["history"])
            eng.mh_set_proposal(update, scales_of(update, delta), kwargs.get("beta", 0.5))
            score_start, score_accept, run_steps, propose = (tuple(bind(eng, M)) + (None,))[:4]
            score_start(U)
        (run_fused if fused else run_step_path)(first, n_mcmc - first)
        if summary:
            self.summary = finalise_summary(eng.chain_summary_read(), n_draws, M)
        self.__dict__.pop("marginals", None)             # a call without marginals= leaves no earlier call's counts behind
        if marg:
            counts = eng.chain_hist_read()
            self.marginals = dict(n=n_draws, chains=M, edges=marg["edges"], hist1d=counts["hist1d"], below=counts["below"],
                                  above=counts["above"], pairs=marg["pairs"], edges2d=marg["edges2d"], hist2d=counts["hist2d"],
                                  outside2d=counts["outside2d"])
        self.__dict__.pop("autocorr", None)              # nor an earlier call's autocorrelations
        if acf:
            self.autocorr = finalise_autocorr(eng.chain_acf_read(), n_draws, M, acf[1], acf[0])
        steps, rate, per = eng.mh_stats(per_chain=True)

        new = np.stack(kept, axis=1) if kept else np.zeros((p, 0, M))      # (p, n_new, M)
        if M == 1:
            new = new[:, :, 0]
        self.samples = new if prev is None else np.concatenate([prev, new], axis=1)
        self.accept = rate
        self.accept_chains = per.astype(np.float64) / max(1, n_mcmc - first)
        self.samples_device = U
        self._mh_next_step = base + n_mcmc

    def _model_mh_device(self, model, n_mcmc, prior, enka, Gamma, delta, enka_scaling, kwargs):
        from .utils import hook_takes_out
        pde = getattr(model, "type", None) == "pde"
        if not hasattr(model, "forward_pde_device" if pde else "forward_device"):
            raise ValueError("chains=: the device path evaluates the forward map on the GPU through model.forward_device, "
                             "which %r does not offer (a 'pde' model offers it as forward_pde_device after "
                             "set_solver(device=True)); run model_mh without chains=" % (model,))
        # fused: None -- the fused chain kernel where the model's map kind has one (FUSED_DEFAULT) --, False, True
        fused = kwargs.get("fused", None)
        if fused not in (None, False, True):
            raise ValueError("fused must be None, False or True, got %r" % (fused,))
        has_fused = (not pde and bool(getattr(model, "fused_kind", False)) and not getattr(model, "flag_noise", False)
                     and hasattr(model, "ensure_installed"))
        if fused and not has_fused:
            raise ValueError("fused=True: %r has no fused chain kernel (ces_amd.utils.elliptic and banana have, noise-free); "
                             "pass fused=None or False for the step path" % (model,))
        leapfrog = self._hmc_leapfrog(kwargs)             # update='hmc': the Langevin proposal, start and default, L positions per test
        langevin = kwargs.get("update", None) in ("langevin", "hmc")      # (model_mh has refused what has no Jacobian)
        default = self.LANGEVIN_FUSED_DEFAULT if langevin else self.FUSED_DEFAULT
        fused = (has_fused and default) if fused is None else bool(fused)
        p, n = enka.p, enka.n_obs

        def scales_of(update, delta=delta):               # exactly as the reference forms them (:122-129)
            if enka_scaling:
                scales = delta * np.linalg.cholesky(np.cov(enka.Ustar).reshape(p, p))
            else:
                scales = delta * np.eye(p)
            return np.linalg.cholesky(prior.cov) if update == "pCN" else scales

        def bind_pde(eng, M):
            # ces/sample.py:133-137, :170-173: every evaluation starts from model.wt at model.t; the start states W are
            # resident and never advanced (the reference keeps w_mcmc fixed), the end states go to a scratch buffer
            import torch
            ns = int(model.n_state)
            wt = np.asarray(model.wt, dtype=np.float64).reshape(ns)
            W = torch.as_tensor(np.ascontiguousarray(np.tile(wt, M).reshape(M, ns).T), device=eng.device)
            W_scratch = torch.empty_like(W)
            G, GP = eng.empty(n), eng.empty(n)

            def fwd(u, out):
                # check=False: nothing is read back; a state whose integration fails has NaN observables
                model.forward_pde_device(eng, u, W, model.t, out=out, W_out=W_scratch, check=False)

            def score_start(U):
                fwd(U, G)
                bad = torch.nonzero(torch.isnan(G).any(dim=0)).reshape(-1)
                if bad.numel():
                    raise ValueError("chains=: the forward model failed at the start state of chain %d (its integration "
                                     "did not finish: no phi to compare a proposal with)" % int(bad[0]))
                eng.mh_start(U, G)

            def score_accept(step, U, P, logu):       # phi(P) NaN for a failed integration: the test rejects (mh_test)
                fwd(P, GP)
                eng.mh_accept(step, U, P, GP, logu=logu)
            return score_start, score_accept, None

        def bind(eng, M):
            takes_out = hook_takes_out(model.forward_device)
            G, GP = eng.empty(n), eng.empty(n)
            if fused:                                     # (a resume that scores no start state: the map is installed all the same)
                model.ensure_installed(eng)

            def fwd(u, out):
                if takes_out:
                    return model.forward_device(eng, u, out=out)
                out.copy_(model.forward_device(eng, u))
                return out

            def score_start(U):
                fwd(U, G)
                eng.mh_start(U, G)

            def score_accept(step, U, P, logu):
                fwd(P, GP)
                eng.mh_accept(step, U, P, GP, logu=logu)

            def run_steps(step, K, U, stride, trace, xi, logu):
                eng.mh_run_map(step, K, U, stride=stride, trace=trace, xi=xi, logu=logu)
            return score_start, score_accept, run_steps if fused else None

        def bind_langevin(eng, M):
            # the map and its Jacobian of one state at a time, fp64: the chains' own g stays in the engine (mh.lv_g)
            import torch
            out = (torch.empty((n, M), dtype=torch.float64, device=eng.device),
                   torch.empty((n, p, M), dtype=torch.float64, device=eng.device))
            model.ensure_installed(eng)

            def lv_start(U):
                model.jacobian_device(eng, U, out=out)
                eng.mh_langevin_start(U, *out)

            def lv_propose(step, U, xi, P):
                eng.mh_langevin_propose(step, U, xi=xi, out=P)

            def lv_accept(step, U, P, logu):
                model.jacobian_device(eng, P, out=out)
                eng.mh_langevin_accept(step, U, P, *out, logu=logu)

            def run_steps(step, K, U, stride, trace, xi, logu):
                eng.mh_langevin_run_map(step, K, U, stride=stride, trace=trace, xi=xi, logu=logu)
            return lv_start, lv_accept, run_steps if fused else None, lv_propose

        def bind_hmc(eng, M, leapfrog=leapfrog, fused=fused):
            # bind_langevin with the leapfrog loop on the host: per position the map and its Jacobian at Q, then the kick
            import torch
            out = (torch.empty((n, M), dtype=torch.float64, device=eng.device),
                   torch.empty((n, p, M), dtype=torch.float64, device=eng.device))
            model.ensure_installed(eng)
            cap = self.HMC_GRADS_MAX // leapfrog

            def hm_start(U):                              # the Langevin start: phi and g of the states
                model.jacobian_device(eng, U, out=out)
                eng.mh_langevin_start(U, *out)

            def hm_begin(step, U, xi, Q):
                eng.mh_hmc_begin(step, U, xi=xi, out=Q)

            def hm_accept(step, U, Q, logu):
                for _ in range(leapfrog - 1):
                    model.jacobian_device(eng, Q, out=out)
                    eng.mh_hmc_leap(Q, *out)
                model.jacobian_device(eng, Q, out=out)
                eng.mh_hmc_accept(step, U, Q, *out, logu=logu)

            def run_steps(step, K, U, stride, trace, xi, logu):
                if K <= cap:
                    eng.mh_hmc_run_map(step, K, leapfrog, U, stride=stride, trace=trace, xi=xi, logu=logu)
                    return 1
                # a trace_stride longer than a launch may be (fused_chunks then makes K = stride: at most one kept state, the
                # last): launches of at most ``cap`` steps without a trace, and the state they leave
                for k0 in range(0, K, cap):
                    k1 = min(K, k0 + cap)
                    eng.mh_hmc_run_map(step + k0, k1 - k0, leapfrog, U, xi=None if xi is None else xi[k0:k1],
                                       logu=None if logu is None else logu[k0:k1])
                if trace is not None and trace.shape[0]:
                    trace[0].copy_(U)
                return -(-K // cap)
            return hm_start, hm_accept, run_steps if fused else None, hm_begin

        def bind_langevin_lineal(eng, M):
            # a linear map (lineal / lineal_log after enable_gradient()): the gradient is an A^T product of the engine's own
            # (cesx_mh_langevin_lineal_*), so a step is the forward map and the engine's launches -- no Jacobian image
            takes_out = hook_takes_out(model.forward_device)
            G, GP = eng.empty(n), eng.empty(n)
            model.langevin_device(eng)

            def fwd(u, out):
                if takes_out:
                    return model.forward_device(eng, u, out=out)
                out.copy_(model.forward_device(eng, u))
                return out

            def lv_start(U):
                fwd(U, G)
                eng.mh_langevin_lineal_start(U, G)

            def lv_propose(step, U, xi, P):
                eng.mh_langevin_lineal_propose(step, U, xi=xi, out=P)

            def lv_accept(step, U, P, logu):
                fwd(P, GP)
                eng.mh_langevin_lineal_accept(step, U, P, GP, logu=logu)
            return lv_start, lv_accept, None, lv_propose

        def bind_hmc_lineal(eng, M, leapfrog=leapfrog):
            # bind_langevin_lineal with the leapfrog loop on the host (cesx_mh_hmc_lineal_*): per position the forward map at Q,
            # then the gradient, the kick and the drift into the OTHER of two position buffers (the drift launch reads Q while it
            # writes the next one).  No fused run: the step is GEMMs
            takes_out = hook_takes_out(model.forward_device)
            G, GQ, Q2 = eng.empty(n), eng.empty(n), eng.empty(p)
            model.langevin_device(eng)

            def fwd(u, out):
                if takes_out:
                    return model.forward_device(eng, u, out=out)
                out.copy_(model.forward_device(eng, u))
                return out

            def hm_start(U):                              # the Langevin start: phi and g of the states
                fwd(U, G)
                eng.mh_langevin_lineal_start(U, G)

            def hm_begin(step, U, xi, Q):
                eng.mh_hmc_lineal_begin(step, U, xi=xi, out=Q)

            def hm_accept(step, U, Q, logu):
                nxt = Q2
                for _ in range(leapfrog - 1):
                    fwd(Q, GQ)
                    eng.mh_hmc_lineal_leap(Q, GQ, nxt)
                    Q, nxt = nxt, Q
                fwd(Q, GQ)
                eng.mh_hmc_lineal_accept(step, U, Q, GQ, logu=logu)
            return hm_start, hm_accept, None, hm_begin

        def darcy_hooks(eng, M):
            # what bind_langevin_darcy and bind_hmc_darcy share: the three outputs of the adjoint launch (G, phi_d, d), fp64, the
            # source of the gradient -- set behind every mh_set_proposal, which returns it to the Jacobian image -- and the start
            import torch
            out = (torch.empty((n, M), dtype=torch.float64, device=eng.device),
                   torch.empty((M,), dtype=torch.float64, device=eng.device),
                   torch.empty((p, M), dtype=torch.float64, device=eng.device))
            model.ensure_installed(eng)
            eng.mh_grad_source("ready")

            def grad(X):                                  # (G, d) at X: a state whose solve failed has NaN in both
                model.gradient_device(eng, X, out=out)
                return out[0], out[2]

            def start(U):
                eng.mh_langevin_start(U, *grad(U))
                bad = torch.nonzero(torch.isnan(out[1])).reshape(-1)          # the one read of a start: phi_d is NaN where the solve failed
                if bad.numel():
                    raise ValueError("chains=: the forward model failed at the start state of chain %d (its system is "
                                     "singular or left fp64's range: no phi and no gradient to compare a proposal with)" % int(bad[0]))
            return grad, start

        def bind_langevin_darcy(eng, M):
            # bind_langevin with the adjoint launch where it forms the Jacobian image (cesx_darcy_grad; cesx_mh_grad_source)
            grad, lv_start = darcy_hooks(eng, M)

            def lv_propose(step, U, xi, P):
                eng.mh_langevin_propose(step, U, xi=xi, out=P)

            def lv_accept(step, U, P, logu):
                eng.mh_langevin_accept(step, U, P, *grad(P), logu=logu)
            return lv_start, lv_accept, None, lv_propose

        def bind_hmc_darcy(eng, M, leapfrog=leapfrog, fused=False):
            # bind_hmc likewise: per position one adjoint launch at Q, then the kick.  No fused run (model_mh has refused fused=True)
            grad, hm_start = darcy_hooks(eng, M)

            def hm_begin(step, U, xi, Q):
                eng.mh_hmc_begin(step, U, xi=xi, out=Q)

            def hm_accept(step, U, Q, logu):
                for _ in range(leapfrog - 1):
                    eng.mh_hmc_leap(Q, *grad(Q))
                eng.mh_hmc_accept(step, U, Q, *grad(Q), logu=logu)
            return hm_start, hm_accept, None, hm_begin

        darcy_grad = langevin and hasattr(model, "gradient_device") and not hasattr(model, "jacobian_device")
        lineal_grad = langevin and not darcy_grad and not hasattr(model, "jacobian_device")      # (a linear map: model_mh has checked langevin_device)
        if darcy_grad:
            bind_langevin = bind_langevin_darcy
            bind_hmc = bind_hmc_darcy
        if lineal_grad:
            bind_langevin = bind_langevin_lineal
            bind_hmc = bind_hmc_lineal
        if leapfrog is not None:
            bind_langevin = bind_hmc
        adapt = self._adapt_of(kwargs, n_mcmc, model)     # (model_mh has refused what it does not go with)
        # a resume under update='langevin' scores the resumed states whatever the noise: the chains need their g as well as phi
        self._mh_device(enka, n_mcmc, prior, kwargs, Gamma, scales_of, bind_langevin if langevin else bind_pde if pde else bind,
                        resume_keeps_start_phi=not langevin, fused=fused, langevin=langevin,
                        fused_steps_max=None if leapfrog is None else self.HMC_GRADS_MAX // leapfrog, adapt=adapt, delta=delta,
                        bind_adapt=(lambda eng, M: bind_hmc_lineal(eng, M, leapfrog or 1)) if lineal_grad else
                        (lambda eng, M: bind_hmc(eng, M, leapfrog or 1, False)),               # (the step path; 'langevin' is L = 1)
                        arm_after_start=lineal_grad)

    def _gp_mh_device(self, enka, n_mcmc, prior, delta, enka_scaling, kwargs):
        import torch
        from . import emulate
        from . import engine as _engine
        host = "; run gp_mh without chains= (the host path)"
        # fused: None -- GP_FUSED_DEFAULT, the step path --, False, True (the fused chain kernel, cesx_gp_run)
        fused = kwargs.get("fused", None)
        if fused not in (None, False, True):
            raise ValueError("fused must be None, False or True, got %r" % (fused,))
        if fused and kwargs.get("separable", False):
            raise ValueError("fused=True: separable predicts one point at a time and has no device path" + host)
        if fused and kwargs.get("pca_tools", None) is not None:
            raise ValueError("fused=True: the dense and the projected Sigma of pca_tools stay on the step path (the fused chain "
                             "kernel scores Gamma, diag(gvars) and diag(Gamma) + diag(gvars)); pass fused=None or False")
        leapfrog = self._hmc_leapfrog(kwargs)             # update='hmc': the Langevin proposal and start, L positions per test
        langevin = kwargs.get("update", None) in ("langevin", "hmc")
        if langevin:
            if fused:
                raise ValueError("fused=True: update=%r runs on the step path (the fused chain kernel has no gradient "
                                 "phase); pass fused=None or False" % (kwargs.get("update"),))
            if leapfrog is None:
                self._langevin_refusals(kwargs, prior)
            else:
                self._as_hmc(self._langevin_refusals, kwargs, prior)
        fused = self.GP_FUSED_DEFAULT if fused is None else bool(fused)
        if kwargs.get("separable", False):
            raise ValueError("chains=: separable predicts one point at a time" + host)
        p, n = enka.p, enka.n_obs
        gpmodels = kwargs.get("gpmodels", None)
        gpmodels = enka.gpmodels if gpmodels is None else gpmodels
        pca = kwargs.get("pca_tools", None)
        Gamma = kwargs.get("Gamma", None)
        n_gp, VD_k, mG, logdet = n, None, None, False
        form = kwargs.get("sigma_form", "dense")
        if form not in ("dense", "projected"):
            raise ValueError("chains=: unknown sigma_form %r ('dense' or 'projected')" % (form,))
        if form == "projected" and pca is None:
            raise ValueError("chains=: sigma_form='projected' projects the Sigma of pca_tools to k x k and needs pca_tools")
        if pca is not None:                               # Sigma = Gamma + VD_k diag(gvars) VD_k^T (:52-53), dense per chain
            if Gamma is None:
                raise ValueError("chains=: pca_tools needs Gamma (the reference adds the (n, n) gvars of pca_tools to it, "
                                 "ces/sample.py:52-53, and cannot run without)")
            if form == "dense" and n > _engine.GP_DENSE_NMAX:
                raise ValueError("chains=: pca_tools factors an n x n Sigma per chain in LDS, n_obs <= %d (got %d)"
                                 % (_engine.GP_DENSE_NMAX, n) + host + ", or pass sigma_form='projected' (k <= %d, any n_obs)"
                                 % _engine.GP_PROJ_KMAX)
            VD_k = np.asarray(pca["VD_k"], dtype=np.float64)
            if VD_k.ndim != 2 or VD_k.shape[0] != n or not 1 <= VD_k.shape[1] <= n:
                raise ValueError("chains=: pca_tools['VD_k'] has shape %s, expected (n_obs, k) = (%d, k <= %d)"
                                 % (VD_k.shape, n, n))
            mG = np.asarray(pca["mG"], dtype=np.float64)
            if mG.shape not in ((n,), (n, 1)):
                raise ValueError("chains=: pca_tools['mG'] has shape %s, expected (%d,) or (%d, 1)" % (mG.shape, n, n))
            mG = mG.reshape(n)
            n_gp = VD_k.shape[1]
            if len(gpmodels) != n_gp:
                raise ValueError("chains=: %d GPs for the k = %d columns of pca_tools['VD_k']" % (len(gpmodels), n_gp))
            logdet = bool(kwargs.get("noise_compounded", False))      # (:69-72)
            mode, G = "dense", np.asarray(Gamma, dtype=np.float64).reshape(n, n)
            if form == "projected":
                if n_gp > _engine.GP_PROJ_KMAX:
                    raise ValueError("chains=: sigma_form='projected' factors a k x k matrix per chain in LDS, k <= %d (got %d)"
                                     % (_engine.GP_PROJ_KMAX, n_gp) + host)
                mode = "proj"
                proj = emulate.project_sigma(G, VD_k, mG, np.asarray(self.y_obs, dtype=np.float64).reshape(n))
        elif len(gpmodels) != n:
            raise ValueError("chains=: %d GPs for n_obs = %d" % (len(gpmodels), n) + host)
        elif Gamma is None:                               # Sigma = diag(gvars) (:48-49)
            mode, G = "var", np.eye(n)
        else:
            G = np.asarray(Gamma, dtype=np.float64).reshape(n, n)
            if kwargs.get("noise_compounded", False):     # Sigma = Gamma + diag(gvars) (:50-51)
                if np.any(G != np.diag(np.diag(G))):
                    raise ValueError("chains=: noise_compounded with a dense Gamma needs a per-chain n x n "
                                     "factorisation" + host)
                mode = "gamma_var"
            else:                                         # Sigma = Gamma (:54-55): the mean alone
                mode = "gamma"
        try:
            img = emulate.device_image(enka, gpmodels)
        except ValueError as exc:
            raise ValueError("chains=: %s" % exc)
        if langevin and np.any(np.asarray(img["family"]) == 1):
            raise ValueError("chains=, update=%r: GP %d has a Matern12 kernel, which is not differentiable at its "
                             "training points; train the emulator with RBF, Matern32 or Matern52"
                             % (kwargs.get("update"), int(np.nonzero(np.asarray(img["family"]) == 1)[0][0])))

        def scales_of(update, delta=delta):               # (:23-26; pCN takes the same scales)
            return delta * np.linalg.cholesky(np.cov(enka.Ustar)) if enka_scaling else delta * np.eye(p)

        def bind(eng, M, leapfrog=leapfrog):
            eng.gp_set(img)
            if mode == "dense":
                eng.gp_dense_set(VD_k, mG, logdet)
            elif mode == "proj":
                eng.gp_proj_set(*proj, logdet)
            nugget, want_var = kwargs.get("nugget", True), mode != "gamma"
            rows = lambda: torch.empty((n_gp, M), dtype=torch.float64, device=eng.device)    # noqa: E731
            mean_u, mean_p = rows(), rows()
            var_u, var_p = (rows(), rows()) if want_var else (None, None)
            if langevin:                                  # the rows and their gradients of one state at a time: the chains' own g stays in the engine
                grads = lambda: torch.empty((n_gp, p, M), dtype=torch.float64, device=eng.device)    # noqa: E731
                out = (mean_p, var_p, grads(), grads() if want_var else None)

                def lv_start(U):
                    eng.gp_predict_grad(U, nugget=nugget, var=want_var, out=out)
                    eng.gp_langevin_start(mode, U, *out)

                def lv_propose(step, U, xi, P):
                    eng.gp_langevin_propose(step, U, xi=xi, out=P)

                def lv_accept(step, U, P, logu):
                    eng.gp_predict_grad(P, nugget=nugget, var=want_var, out=out)
                    eng.gp_langevin_accept(mode, step, U, P, *out, logu=logu)

                def hm_begin(step, U, xi, Q):             # update='hmc': the same start, then per position the rows at Q and the kick
                    eng.mh_hmc_begin(step, U, xi=xi, out=Q)

                def hm_accept(step, U, Q, logu):
                    for _ in range(leapfrog - 1):
                        eng.gp_predict_grad(Q, nugget=nugget, var=want_var, out=out)
                        eng.gp_hmc_leap(mode, Q, *out)
                    eng.gp_predict_grad(Q, nugget=nugget, var=want_var, out=out)
                    eng.gp_hmc_accept(mode, step, U, Q, *out, logu=logu)
                if leapfrog is not None:
                    return lv_start, hm_accept, None, hm_begin
                return lv_start, lv_accept, None, lv_propose

            def score_start(U):
                eng.gp_predict(U, nugget=nugget, var=want_var, out=(mean_u, var_u))
                eng.gp_start(mode, U, mean_u, var_u)

            def score_accept(step, U, P, logu):
                eng.gp_predict(P, nugget=nugget, var=want_var, out=(mean_p, var_p))
                eng.gp_accept(mode, step, U, P, mean_p, var_p, logu=logu)

            def run_steps(step, K, U, stride, trace, xi, logu):
                try:
                    eng.gp_run(mode, step, K, U, stride=stride, trace=trace, xi=xi, logu=logu, nugget=nugget)
                except _engine.CesxError as exc:
                    if exc.code != _engine.EUNSUPPORTED:
                        raise
                    raise ValueError("chains=, fused=True: %s -- the fused chain kernel keeps a tile's K* panel, GP rows and "
                                     "states in LDS, 256 (3 p + J_p + 2 n_gp) + 8192 bytes <= 160 KiB; pass fused=False for the "
                                     "step path" % exc)
            return score_start, score_accept, run_steps if fused else None

        # the arithmetic of one fused step of all chains, in the units of GP_FUSED_WORK
        Jp = (int(img["Jt"]) + 15) // 16 * 16
        work = int(kwargs["chains"]) * n_gp * Jp * (Jp // 2 + p + 8) if fused else 0
        self._mh_device(enka, n_mcmc, prior, kwargs, G, scales_of, bind, resume_keeps_start_phi=False, fused=fused,
                        fused_work=work, langevin=True, adapt=self._adapt_of(kwargs, n_mcmc), delta=delta,
                        bind_adapt=lambda eng, M: bind(eng, M, leapfrog or 1))      # (the leapfrog hooks; 'langevin' is L = 1)
