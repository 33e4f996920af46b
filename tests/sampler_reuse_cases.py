"""One Sample-stage engine across every change of update (tests/test_sampler_reuse_host.py, tests/test_gpu_sampler_reuse.py).

Production reuses ``MhState``: ``MCMC._mh_engine`` keeps one engine per (p, n_obs, chains, dtype, device, seed) and every later
``model_mh`` / ``gp_mh`` call runs on the memory the previous call left -- the noise block, g, the momenta, z, a / b, phi, the
counters, the adaptation state, the chain-statistics stages.  This module holds

  * the BLOCK tables: a block is one sampler on one engine -- set_problem, mh_set_proposal, the installs, the start, ``STEPS``
    steps with the call order of the ``bind*`` hooks of ces_amd/sample.py, a read-back of U, phi and the per-chain counters and,
    for the gradient samplers, one more step and a second read-back (g of the last accept then has an observable effect);
  * the generated SEQUENCES of blocks on ONE engine (pair cover, NaN polluters, abandoned work) and the runner: the twin of a
    block is the same block on a freshly created engine with the same shape, dtype, seed and step indices, and the two are
    compared as bytes;
  * the cross-family CALL-ORDER table of the Sample and Emulate step entry points, derived from the prose of include/cesx.h.

Everything but ``run_block``, ``Hooks`` and ``stats_use`` imports and runs without a device."""
import functools
import os
import re
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import adapt_cases as ac  # noqa: E402
import gp_chain_cases as gcc  # noqa: E402
import gp_dense_cases as gdc  # noqa: E402
import gp_langevin_cases as glc  # noqa: E402
import hmc_cases as hc  # noqa: E402
import lineal_hmc_cases as lhc  # noqa: E402
import lineal_langevin_cases as llc  # noqa: E402
import map_cases as mc_  # noqa: E402
import map_langevin_cases as mlc  # noqa: E402
from gp_cases import random_gps  # noqa: E402

# 130 chains: two waves and a ragged third; the closed-form maps need p = n_obs = 2.  257: four waves and one chain.
ENGINES = {"A": dict(p=2, n=2, J=130, k=2), "B": dict(p=3, n=5, J=257, k=3)}
DTYPES = ("float64", "float32")
SEED = 2024                    # the engines' seed: the device noise of step s is Philox(SEED, s)
STEPS = 3
JT, FAMILY = 17, "Matern32"
A_STEPS, POST_STEPS = 3, 2     # adaptation steps; steps behind the join
GAIN, KAPPA = ac.GAIN, ac.KAPPA
NOISES = ("device", "injected")
GP_HMC_DELTA = 0.12            # the emulator's leapfrog step (fp64 numpy accepts 0.9 .. 0.99 of 4 steps: not every chain moves every time)


def _k(fam, sampler, engines="AB", **kw):
    d = dict(fam=fam, sampler=sampler, engines=engines, L=None, fused=False, adapt=0, mode=None, pcn=False, log=False)
    d.update(kw)
    return d


# fam: 'fwd' the random walk on a forward model (A: elliptic / banana, B: a linear map), 'gp' the emulator, 'map' a closed-form map
# with its Jacobian, 'lin' a linear map through the adjoint images.  sampler: 'rw' | 'lv' | 'hmc'.
KINDS = {
    "rw": _k("fwd", "rw"),
    "pcn": _k("fwd", "rw", pcn=True),
    "rw_fused": _k("fwd", "rw", "A", fused=True),
    "gp_gamma": _k("gp", "rw", mode="gamma"),
    "gp_var": _k("gp", "rw", mode="var"),
    "gp_gamma_var": _k("gp", "rw", mode="gamma_var"),
    "gp_dense": _k("gp", "rw", mode="dense"),
    "gp_proj": _k("gp", "rw", mode="proj"),
    "gp_run": _k("gp", "rw", mode="gamma", fused=True),
    "gp_lv": _k("gp", "lv", mode="gamma_var"),
    "gp_hmc": _k("gp", "hmc", mode="gamma", L=3),
    "gp_proj_lv": _k("gp", "lv", mode="proj"),
    "gp_proj_hmc": _k("gp", "hmc", mode="proj", L=3),
    "map_lv": _k("map", "lv", "A"),
    "map_lv_fused": _k("map", "lv", "A", fused=True),
    "map_hmc": _k("map", "hmc", "A", L=3),
    "map_hmc_fused": _k("map", "hmc", "A", L=3, fused=True),
    "lin_lv": _k("lin", "lv"),
    "log_lv": _k("lin", "lv", log=True),
    "lin_hmc": _k("lin", "hmc", L=3),
    "adapt_map": _k("map", "hmc", "A", L=3, adapt=A_STEPS),
    "adapt_gp": _k("gp", "hmc", mode="gamma_var", L=1, adapt=A_STEPS),       # (update='langevin' adapts as L = 1)
    "adapt_lin": _k("lin", "hmc", L=2, adapt=A_STEPS),
}

# What include/cesx.h refuses on an fp32 engine alone, kind -> the sentence: those blocks leave the fp32 tables.  The header
# states no such refusal for the Sample and Emulate stages (an fp32 engine "rounds where it stores"; every sum is fp64), so the
# fp32 tables are the fp64 ones; tests/test_sampler_reuse_host.py holds the header to that.
FP32_REFUSED = {}
FP32_ENGINE_WORDS = re.compile(r"fp32|fp64 engine|float32|CESX_F32|CESX_F64|single precision|engine dtype", re.I)
FP32_REFUSAL_WORDS = re.compile(r"CESX_E[A-Z]+|refus|unsupported|not supported|cannot|can not|does not take|is not offered|needs an? fp64|"
                                r"fp64 (engines? )?only|only (on|for|with) (an? )?fp64", re.I)


def fp32_refusal_sentences(text):
    """The sentences of ``text`` that speak of an engine dtype AND of a refusal, whatever their wording: a sentence ends at a full
    stop followed by space, at a semicolon or at the end of a comment."""
    flat = " ".join(text.replace("*/", ". ").split())
    return [t for t in re.split(r"(?<=[.;])\s+", flat) if FP32_ENGINE_WORDS.search(t) and FP32_REFUSAL_WORDS.search(t)]


def kinds_of(E, dtype="float64"):
    out = [k for k, d in KINDS.items() if E in d["engines"]]
    if dtype == "float32":
        out = [k for k in out if k not in FP32_REFUSED]
    return out


def gradient(kind):
    return KINDS[kind]["sampler"] in ("lv", "hmc")


def polluters(E, dtype="float64"):
    """The gradient kinds whose forward output the caller hands in (a fused launch evaluates its map itself)."""
    return [k for k in kinds_of(E, dtype) if gradient(k) and not KINDS[k]["fused"]]


# ---- problems ------------------------------------------------------------------------------------------------------------------

def _rng(*key):
    return np.random.default_rng(zlib.crc32("/".join(str(k) for k in key).encode()))


def _lin_problem(E, log, prob, dense_prior=False):
    """A linear problem at the engine's (p, n_obs) in the dict form and by the recipe of ``lineal_langevin_cases.problem`` (its
    numpy chains take any such dict).  That module's 'lineal-5x3' / 'log-5x3' are p = 5, n_obs = 3 and do not fit engine B's
    (3, 5), which the five-GP emulator and k = 3 fix; B hosts the same recipe at p = 3, n_obs = 5.  Gamma is dense in problem 0
    and diagonal in problem 1, the prior the other way round (``dense_prior``: dense in both)."""
    rng = _rng("lin", E, log, prob)
    p, n = ENGINES[E]["p"], ENGINES[E]["n"]
    A = rng.uniform(0.2, 1.0, (n, p)) / p if log else rng.standard_normal((n, p)) / np.sqrt(p) + np.eye(n, p)
    b = 0 if log else 0.5 * rng.standard_normal(n)
    Gamma = llc._spd(rng, n, 0.05) if prob == 0 else np.diag(rng.uniform(0.05, 0.2, n))
    Sigma = np.diag(rng.uniform(0.5, 2.0, p)) if prob == 0 and not dense_prior else llc._spd(rng, p, 0.5 + prob)
    mu = 0.3 * rng.standard_normal(p) + prob
    u_true = mu + 0.5 * np.linalg.cholesky(Sigma) @ rng.standard_normal(p)
    Ex = np.exp(u_true) if log else u_true
    y = A @ Ex + b + np.linalg.cholesky(Gamma) @ rng.standard_normal(n)
    Gi, Si = np.linalg.inv(Gamma), np.linalg.inv(Sigma)
    Jm = A * np.exp(u_true)[None, :] if log else A
    C = np.linalg.inv(Jm.T @ Gi @ Jm + Si)
    C = 0.5 * (C + C.T)
    m = u_true if log else C @ (A.T @ Gi @ (y - b) + Si @ mu)
    ens = m[:, None] + np.linalg.cholesky(C) @ rng.standard_normal((p, 130))
    return dict(name="%s-%dx%d-%d" % ("log" if log else "lineal", n, p, prob), kind="lineal_log" if log else "lineal", p=p, n=n, A=A, b=b,
                Gamma=Gamma, Sigma=Sigma, mu=mu, y=y, ens=ens, delta=0.5 if log else 0.8, m=m, C=C)


@functools.lru_cache(maxsize=None)
def spec(E, kind, prob):
    """Everything a block of ``kind`` on engine ``E`` needs of problem ``prob`` (0 | 1), host fp64.  The two problems of a kind
    differ in y, in Gamma (dense in one, diagonal in the other, but for the kinds that need one of the two), in the prior and in
    the scale of the start states."""
    d, e = KINDS[kind], ENGINES[E]
    p, n, J = e["p"], e["n"], e["J"]
    rng = _rng("spec", E, kind, prob)
    sp = dict(E=E, kind=kind, prob=prob, p=p, n=n, J=J, fam=d["fam"], sampler=d["sampler"], L=d["L"], fused=d["fused"],
              adapt=d["adapt"], beta=0.5, mode=d["mode"], lin=None, gp=None, mapkind=None,
              base=1000 * (list(KINDS).index(kind) + 1) + 100 * prob + 7,           # the block's first step index
              noise_seed=zlib.crc32(("noise/%s/%s/%d" % (E, kind, prob)).encode()) % (2 ** 31))
    spread = sp["spread"] = (1.0, 0.4)[prob]            # the scale of the start states about their centre
    if d["fam"] == "map" or (d["fam"] == "fwd" and E == "A"):
        mk = ("elliptic", "banana")[prob]
        model, y, Gamma, mean, cov, _ = mc_.problem(mk, None)            # elliptic: a diagonal Gamma, banana: a dense one; dense priors
        sp.update(mapkind=mk, y=y, Gamma=Gamma, mu=mean, cov=cov)
        C, delta = np.linalg.cholesky(np.cov(mc_.start_ensemble(mk, 130, np.random.default_rng(4)))), mlc.DELTA[mk]
        if d["sampler"] == "hmc":
            delta *= 0.5
        ens = mc_.start_ensemble(mk, J, _rng("ens", E, kind, prob))
        sp["U0"] = ens.mean(axis=1)[:, None] + spread * (ens - ens.mean(axis=1)[:, None])
        if d["pcn"]:
            C, delta, sp["beta"] = np.linalg.cholesky(cov), 1.0, mc_.BETA[mk]
    elif d["fam"] in ("lin", "fwd"):
        lp = _lin_problem(E, d["log"], prob, dense_prior=d["fam"] == "fwd")
        sp.update(lin=lp, y=lp["y"], Gamma=lp["Gamma"], mu=lp["mu"], cov=lp["Sigma"])
        C, delta = np.linalg.cholesky(np.cov(lp["ens"]).reshape(p, p)), lp["delta"]
        if d["sampler"] == "hmc":
            delta *= 0.5
        sp["U0"] = lp["m"][:, None] + spread * (np.linalg.cholesky(lp["C"]) @ rng.standard_normal((p, J)))
        if d["pcn"]:
            C, delta, sp["beta"] = np.linalg.cholesky(lp["Sigma"]), 1.0, 0.3
    else:
        mode = d["mode"]
        if mode in ("dense", "proj"):
            k = e["k"]
            enka = random_gps(rng, p, k, JT, FAMILY, scaled=bool(prob))
            pr = gdc.problem(rng, n, k, 1e2, "pca", p=p, dense_prior=prob == 0)
            if prob == 1:
                pr["Gamma"] = np.diag(np.diag(pr["Gamma"]))
            logdet = prob == 0
            sp.update(y=pr["y"], Gamma=pr["Gamma"], mu=enka.Ustar.mean(axis=1) + pr["mu"], cov=pr["Sp"],
                      gp=dict(enka=enka, nugget=True, B=pr["B"], g0=pr["g0"], logdet=logdet, c=None))
            delta = 0.3
        else:
            # the case tables of tests/gp_chain_cases.py at this engine's shape: its numpy chains rebuild the problem from `c`
            gmode = "gamma_dense" if mode == "gamma" and prob == 1 else mode
            prior = "rw_dense" if prob == 0 else ("pcn" if kind == "gp_var" else "rw_diag")
            c = dict(M=J, Jt=JT, p=p, n=n, family=FAMILY, nugget=prob == 0, mode=gmode, prior=prior,
                     seed=200 + 2 * list(KINDS).index(kind) + prob)
            enka, y, pri, kw = gcc.problem(c)
            Gamma = kw.get("Gamma", None)
            sp.update(y=y, Gamma=np.eye(n) if Gamma is None else Gamma, mu=np.asarray(pri.mean), cov=np.asarray(pri.cov).reshape(p, p),
                      gp=dict(enka=enka, nugget=kw["nugget"], c=c, kw=kw, prior=pri, Gamma=Gamma), beta=kw.get("beta", 0.5))
            d = dict(d, pcn=kw.get("update") == "pCN" and d["sampler"] == "rw")
            delta = kw["delta"]
        C = np.linalg.cholesky(np.cov(enka.Ustar))
        if d["sampler"] == "lv":
            delta = 0.2
        elif d["sampler"] == "hmc":
            delta = GP_HMC_DELTA
        sp["U0"] = enka.Ustar.mean(axis=1)[:, None] + 0.2 * spread * rng.standard_normal((p, J))
    sp["update"] = "pCN" if d["pcn"] else None if d["sampler"] == "rw" else "langevin"
    sp["C"], sp["delta"] = C, float(delta)
    sp["S"] = delta * C
    sp["target"] = ac.TARGET["langevin" if d["L"] == 1 else "hmc"]
    return sp


def n_steps(kind, variant=None):
    """The steps a block of ``kind`` makes, whatever the variant breaks off (its injected draws are cut from this many)."""
    d = KINDS[kind]
    return d["adapt"] + POST_STEPS if d["adapt"] else STEPS + (1 if gradient(kind) else 0)


def injected(sp, count=None):
    """The block's injected draws in the order of noise='numpy': per step normal(0, 1, [p, J]), then log(uniform(J))."""
    rs = np.random.RandomState(sp["noise_seed"])
    xi, lu = [], []
    for _ in range(n_steps(sp["kind"]) if count is None else count):
        xi.append(rs.normal(0, 1, [sp["p"], sp["J"]]))
        lu.append(np.log(rs.uniform(size=sp["J"])))
    return np.array(xi), np.array(lu)


# ---- sequences -----------------------------------------------------------------------------------------------------------------
# An item is (kind, problem, noise, variant): variant None, 'nan' (the last step is handed non-finite forward output in every
# column), 'ab_propose' (a propose without its accept), 'ab_leap' (hmc begin and one leap, no accept) or 'ab_adapt' (armed, one
# of A_STEPS adaptation steps made, never read).

def _alt(i):
    return i % 2, NOISES[(i // 2) % 2]


def pair_cover(E, dtype, first):
    """The part of the pair cover that starts with ``first``: X Y X Y' X .. over the kinds Y from X on in table order, X last on
    its other problem -- the pairs (X, Y) and (Y, X) for every Y >= X, (X, X) included.  The parts of all X together hold
    every ordered pair of the engine's kinds."""
    kinds = kinds_of(E, dtype)
    i0 = kinds.index(first)
    seq = []
    for t, Y in enumerate(kinds[i0 + 1:]):
        seq.append((first, t % 2, NOISES[t % 2], None))
        seq.append((Y, (t // 2) % 2, NOISES[(t + 1) % 2], None))
    seq.append((first, 0, "device", None))
    seq.append((first, 1, "injected", None))
    seq.append((first, 0, "injected", None))
    return seq


def pairs_in(seq):
    return {(a[0], b[0]) for a, b in zip(seq, seq[1:])}


def nan_cover(E, dtype, polluter):
    """``polluter`` with its last step poisoned, in front of every kind once."""
    seq = []
    for t, Y in enumerate(kinds_of(E, dtype)):
        seq.append((polluter, t % 2, NOISES[(t // 2) % 2], "nan"))
        seq.append((Y, (t + 1) % 2, NOISES[t % 2], None))
    return seq


ABANDON_FORMS = ("ab_propose", "ab_leap", "ab_adapt")


def abandoners(E, dtype, form):
    kinds = kinds_of(E, dtype)
    if form == "ab_propose":          # the samplers with a propose call of their own
        return [k for k in kinds if not KINDS[k]["fused"] and not KINDS[k]["adapt"] and KINDS[k]["sampler"] != "hmc"]
    if form == "ab_leap":
        return [k for k in kinds if not KINDS[k]["fused"] and not KINDS[k]["adapt"] and KINDS[k]["sampler"] == "hmc"]
    return [k for k in kinds if KINDS[k]["adapt"]]


def abandon_cover(E, dtype, form):
    """An interrupted block in front of every kind once; the interrupted kinds go round robin."""
    who = abandoners(E, dtype, form)
    seq = []
    for t, Y in enumerate(kinds_of(E, dtype)):
        seq.append((who[t % len(who)], t % 2, NOISES[(t // 2) % 2], form))
        seq.append((Y, (t + 1) % 2, NOISES[t % 2], None))
    return seq


# ---- the runner (device) ---------------------------------------------------------------------------------------------------------

class Hooks:
    """The hooks of ``MCMC._model_mh_device`` / ``_gp_mh_device``'s ``bind*`` for one block: ``start(U)``, ``propose(step, U, xi,
    P)`` (the begin of a trajectory for 'hmc'), ``accept(step, U, P, logu)``, ``run(step, K, U, xi, logu)`` for the fused kinds and
    ``leap(Q)`` (one position of a trajectory).  ``poison = True``: every forward output handed to the engine is NaN in every
    column, and the forward kernels are not launched on the positions that follow from it."""

    def __init__(self, eng, sp, leapfrog=None):
        import torch
        from ces_amd import emulate, utils
        self.eng, self.sp, self.poison = eng, sp, False
        self.L = leapfrog if leapfrog is not None else sp["L"]
        p, n, J = sp["p"], sp["n"], sp["J"]
        f64 = lambda *s: torch.empty(s, dtype=torch.float64, device=eng.device)      # noqa: E731
        self.fam = fam = sp["fam"]
        if fam == "gp":
            g = sp["gp"]
            if "img" not in g:
                g["img"] = emulate.device_image(g["enka"], g["enka"].gpmodels)
            img = g["img"]
            eng.gp_set(img)
            self.mode = mode = sp["mode"]
            if mode == "dense":
                eng.gp_dense_set(g["B"], g["g0"], g["logdet"])
            elif mode == "proj":
                eng.gp_proj_set(*emulate.project_sigma(sp["Gamma"], g["B"], g["g0"], sp["y"]), g["logdet"])
            k = int(img["n"])
            self.nugget, self.want_var = g["nugget"], mode != "gamma"
            self.rows_u = (f64(k, J), f64(k, J) if self.want_var else None)
            self.rows_p = (f64(k, J), f64(k, J) if self.want_var else None)
            self.out = (self.rows_p[0], self.rows_p[1], f64(k, p, J), f64(k, p, J) if self.want_var else None)
        elif fam == "lin" or (fam == "fwd" and sp["lin"] is not None):
            lp = sp["lin"]
            self.model = utils.lineal(lp["A"], lp["b"]) if lp["kind"] == "lineal" else utils.lineal_log(lp["A"])
            self.G, self.GP, self.Q2 = eng.empty(n), eng.empty(n), eng.empty(p)
            if fam == "lin":
                self.model.enable_gradient(leapfrog=sp["sampler"] == "hmc")
                self.model.langevin_device(eng)
        else:
            self.model = utils.elliptic() if sp["mapkind"] == "elliptic" else utils.banana()
            self.G, self.GP = eng.empty(n), eng.empty(n)
            self.out = (f64(n, J), f64(n, p, J))
            if sp["fused"] or fam == "map":
                self.model.ensure_installed(eng)

    # -- forward outputs: the rows and gradients at X into self.out (gp, map) or G (lin, fwd) --
    def _nan(self, ts):
        for t in ts:
            if t is not None:
                t.fill_(float("nan"))

    def _grad(self, X):
        if self.poison:                   # the emulator: mean and dmean; a map: G and DG
            return self._nan((self.out[0], self.out[2]) if self.fam == "gp" else self.out)
        if self.fam == "gp":
            self.eng.gp_predict_grad(X, nugget=self.nugget, var=self.want_var, out=self.out)
        else:
            self.model.jacobian_device(self.eng, X, out=self.out)

    def _fwd(self, X, out):
        if self.poison:
            return self._nan((out,))
        self.model.forward_device(self.eng, X, out=out)

    def start(self, U):
        eng, sp = self.eng, self.sp
        if sp["sampler"] == "rw":
            if self.fam == "gp":
                eng.gp_predict(U, nugget=self.nugget, var=self.want_var, out=self.rows_u)
                eng.gp_start(self.mode, U, *self.rows_u)
            else:
                self._fwd(U, self.G)
                eng.mh_start(U, self.G)
        elif self.fam == "gp":
            self._grad(U)
            eng.gp_langevin_start(self.mode, U, *self.out)
        elif self.fam == "map":
            self._grad(U)
            eng.mh_langevin_start(U, *self.out)
        else:
            self._fwd(U, self.G)
            eng.mh_langevin_lineal_start(U, self.G)

    def propose(self, step, U, xi, P):
        eng, s = self.eng, self.sp["sampler"]
        if s == "rw":
            eng.mh_propose(step, U, xi=xi, out=P)
        elif self.fam == "lin":
            (eng.mh_hmc_lineal_begin if s == "hmc" else eng.mh_langevin_lineal_propose)(step, U, xi=xi, out=P)
        elif s == "hmc":
            eng.mh_hmc_begin(step, U, xi=xi, out=P)
        elif self.fam == "gp":
            eng.gp_langevin_propose(step, U, xi=xi, out=P)
        else:
            eng.mh_langevin_propose(step, U, xi=xi, out=P)

    def leap(self, Q):
        """One position of a trajectory; returns the buffer that holds the next one."""
        eng = self.eng
        if self.fam == "lin":
            nxt = self.Q2 if Q is not self.Q2 else self._Q1
            self._fwd(Q, self.GP)
            eng.mh_hmc_lineal_leap(Q, self.GP, nxt)
            return nxt
        self._grad(Q)
        if self.fam == "gp":
            eng.gp_hmc_leap(self.mode, Q, *self.out)
        else:
            eng.mh_hmc_leap(Q, *self.out)
        return Q

    def accept(self, step, U, P, logu):
        eng, s = self.eng, self.sp["sampler"]
        if s == "hmc":
            self._Q1 = P
            for _ in range(self.L - 1):
                P = self.leap(P)
        if s == "rw":
            if self.fam == "gp":
                eng.gp_predict(P, nugget=self.nugget, var=self.want_var, out=self.rows_p)
                eng.gp_accept(self.mode, step, U, P, *self.rows_p, logu=logu)
            else:
                self._fwd(P, self.GP)
                eng.mh_accept(step, U, P, self.GP, logu=logu)
        elif self.fam == "gp":
            self._grad(P)
            (eng.gp_hmc_accept if s == "hmc" else eng.gp_langevin_accept)(self.mode, step, U, P, *self.out, logu=logu)
        elif self.fam == "map":
            self._grad(P)
            (eng.mh_hmc_accept if s == "hmc" else eng.mh_langevin_accept)(step, U, P, *self.out, logu=logu)
        else:
            self._fwd(P, self.GP)
            (eng.mh_hmc_lineal_accept if s == "hmc" else eng.mh_langevin_lineal_accept)(step, U, P, self.GP, logu=logu)

    def run(self, step, K, U, xi, logu):
        eng, s = self.eng, self.sp["sampler"]
        if self.fam == "gp":
            eng.gp_run(self.mode, step, K, U, xi=xi, logu=logu, nugget=self.nugget)
        elif s == "rw":
            eng.mh_run_map(step, K, U, xi=xi, logu=logu)
        elif s == "lv":
            eng.mh_langevin_run_map(step, K, U, xi=xi, logu=logu)
        else:
            eng.mh_hmc_run_map(step, K, self.L, U, xi=xi, logu=logu)


def read_back(eng, U):
    steps, _, per = eng.mh_stats(per_chain=True)
    return dict(U=U.cpu().numpy().copy(), phi=eng.mh_phi(), cnt=per.copy(), steps=np.array([steps]))


def run_block(eng, sp, noise, variant=None, mid=None, first_step=None, U0=None):
    """One block on ``eng``; returns the read-backs as a flat dict of numpy arrays (``differences`` compares two of them as
    bytes).  ``mid``: called once behind the block's first step (the chain statistics in the middle of a block).
    ``first_step`` / ``U0``: the controls' displaced step index and start states."""
    import torch
    p = sp["p"]
    base = sp["base"] if first_step is None else first_step
    total = n_steps(sp["kind"])
    xi_h = lu_h = None
    if noise == "injected":
        xi_h, lu_h = injected(sp)
        xi_d = torch.as_tensor(xi_h, device=eng.device).to(eng.torch_dtype).contiguous()
        lu_d = torch.as_tensor(lu_h, dtype=torch.float64, device=eng.device).contiguous()
    noise_of = lambda k, K=None: ((None, None) if xi_h is None else                      # noqa: E731
                                  (xi_d[k], lu_d[k]) if K is None else (xi_d[k:k + K].contiguous(), lu_d[k:k + K].contiguous()))
    out = {}
    eng.set_problem(sp["y"], sp["Gamma"], sp["mu"], sp["cov"], sp["mu"])
    eng.mh_set_proposal(sp["update"], sp["S"], sp["beta"])
    A, lin = sp["adapt"], sp["fam"] == "lin"
    arm = lambda: eng.mh_adapt_set(A, sp["target"], GAIN, KAPPA)      # noqa: E731
    if A and not lin:                  # (armed before the hooks and the start, as the models with a Jacobian and the emulator take it)
        arm()
    hk = Hooks(eng, sp)
    U = eng.to_device(np.asarray(sp["U0"] if U0 is None else U0, dtype=np.float64), p, "mh_U").clone()
    P = eng.empty(p)
    hk.start(U)
    out["r0_phi"] = eng.mh_phi()       # phi of the start states
    if A and lin:                      # (the linear maps' install and start refuse an armed handle)
        arm()

    def step(k, poison=False):
        xi, lu = noise_of(k)
        hk.poison = poison
        hk.propose(base + k, U, xi, P)
        hk.accept(base + k, U, P, lu)
        hk.poison = False

    if variant in ("ab_propose", "ab_leap", "ab_adapt"):
        step(0)
        if variant == "ab_propose":
            hk.propose(base + 1, U, noise_of(1)[0], P)
        elif variant == "ab_leap":
            hk.propose(base + 1, U, noise_of(1)[0], P)
            hk._Q1 = P
            hk.leap(P)
        out.update({"ab_" + k: v for k, v in read_back(eng, U).items()})
        return out
    if A:
        for k in range(A):
            step(k)
        found = eng.mh_adapt_read()
        out.update(multiplier=np.array([found["multiplier"]]), history=found["history"], U_adapt=U.cpu().numpy().copy())
        eng.mh_set_proposal(sp["update"], (sp["delta"] * found["multiplier"]) * sp["C"], sp["beta"])
        hk = Hooks(eng, sp)
        hk.start(U)
        for k in range(A, total):
            if k == total - 1:             # in front of the last step: what a poisoned one must leave as it is
                out.update({"pre_" + key: v for key, v in read_back(eng, U).items()})
            step(k, poison=variant == "nan" and k == total - 1)
            if mid is not None and k == A:
                mid(U)
        out.update(read_back(eng, U))
        return out
    if sp["fused"]:
        hk.run(base, STEPS, U, *noise_of(0, STEPS))
        rb = read_back(eng, U)
        out.update({"r3_" + k: v for k, v in rb.items()})
        if mid is not None:
            mid(U)
        if gradient(sp["kind"]):
            hk.run(base + STEPS, 1, U, *noise_of(STEPS, 1))
            rb = read_back(eng, U)
        out.update(rb)
        return out
    for k in range(STEPS):
        step(k)
        if mid is not None and k == 0:
            mid(U)
    rb = read_back(eng, U)
    out.update({"r3_" + k: v for k, v in rb.items()})
    if gradient(sp["kind"]):
        step(STEPS, poison=variant == "nan")
        rb = read_back(eng, U)
    out.update(rb)
    return out


def differences(a, b):
    """The comparator: the keys of two read-backs whose arrays are not equal as bytes (a missing key differs)."""
    bad = []
    for k in sorted(set(a) | set(b)):
        if k not in a or k not in b:
            bad.append(k)
            continue
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        if x.dtype != y.dtype or x.shape != y.shape or x.tobytes() != y.tobytes():
            bad.append(k)
    return bad


# ---- chain statistics between and inside the blocks -----------------------------------------------------------------------------

def stats_plan(E, i):
    """Use ``i`` of the three chain-statistics stages: N, the chunking, bins and pairs, lags and followed chains all vary."""
    e = ENGINES[E]
    p, J = e["p"], e["J"]
    N = (6, 9, 4, 12, 7)[i % 5]
    return dict(N=N, chunks=((N,), (1, N - 1), (2, 1, N - 3), (N - 2, 2))[i % 4], bins=(4, 7, 3, 16)[i % 4], bins2=(3, 5)[i % 2],
                pairs=((), ((0, 1),), ((1, 0), (0, p - 1)))[i % 3], lags=(1, 2, 2, 3, 5)[i % 5], chains=(1, J, 33, 64, J - 1)[i % 5],
                abandoned=i % 3 == 1, seed=900 + i)


def stats_draws(E, plan, dtype):
    e = ENGINES[E]
    rng = np.random.default_rng(plan["seed"])
    return (rng.standard_normal((plan["N"], e["p"], e["J"])) * (1 + plan["seed"] % 3)).astype(dtype)


def stats_use(eng, E, i, abandoned=None):
    """One use of every stage on ``eng``; with ``abandoned`` (None: the plan's) a run that is begun, given fewer than N draws and
    never read goes in front.  The fresh baseline passes False: the read behind an abandoned run is held to a run that never had
    one.  Returns the reads as a flat dict."""
    import torch
    plan = stats_plan(E, i)
    p = ENGINES[E]["p"]
    draws = torch.as_tensor(stats_draws(E, plan, eng.np_dtype), device=eng.device).contiguous()
    edges = lambda b: np.tile(np.linspace(-3.0, 3.0, b + 1) * (1 + 0.1 * i), (p, 1)) + np.arange(p)[:, None] * 0.01      # noqa: E731
    pairs = np.asarray(plan["pairs"], dtype=np.int32).reshape(-1, 2)
    if plan["abandoned"] if abandoned is None else abandoned:
        eng.chain_summary_begin(plan["N"] + 3)
        eng.chain_summary_add(draws[:2].contiguous())
        eng.chain_hist_begin(edges(plan["bins"] + 1), edges(plan["bins2"]), [(0, 1)])
        eng.chain_hist_add(draws[:2].contiguous())
        eng.chain_acf_begin(plan["N"] + 3, plan["lags"], max(1, plan["chains"] // 2))
        eng.chain_acf_add(draws[:2].contiguous())
    eng.chain_summary_begin(plan["N"])
    eng.chain_hist_begin(edges(plan["bins"]), edges(plan["bins2"]) if len(pairs) else None, pairs if len(pairs) else None)
    eng.chain_acf_begin(plan["N"], plan["lags"], plan["chains"])
    t = 0
    for c in plan["chunks"]:
        if c < 1:
            continue
        blk = draws[t:t + c].contiguous()
        eng.chain_summary_add(blk)
        eng.chain_hist_add(blk)
        eng.chain_acf_add(blk)
        t += c
    assert t == plan["N"]
    out = {}
    out.update({"sum_" + k: v for k, v in eng.chain_summary_read(halves=True).items()})
    out.update({"hist_" + k: v for k, v in eng.chain_hist_read().items()})
    out.update({"acf_" + k: v for k, v in eng.chain_acf_read(chains=True).items()})
    return out


# ---- the blocks against the features' own numpy chains ----------------------------------------------------------------------------
# kind -> what stands behind it.  None: no numpy chain exists at these shapes (NOTEBOOK.md lists them).

def has_reference(E, kind, noise, dtype):
    d = KINDS[kind]
    if d["fam"] == "gp" and d["sampler"] == "rw":
        # gp_chain_cases.np_chains: the device noise, fp64, the modes of the fused kernel
        return d["mode"] in ("gamma", "var", "gamma_var") and noise == "device" and dtype == "float64"
    if d["sampler"] == "rw" or d["mode"] == "proj":
        return False
    if d["adapt"]:
        return noise == "injected" and dtype == "float64"
    return noise == "injected"


def reference(sp):
    """(U, accepted per chain[, adapt dict]) of the block's steps in the feature's fp64 numpy chain; the injected kinds draw from
    the global RNG under the block's noise seed, exactly what ``injected`` hands the engine."""
    kind, d = sp["kind"], KINDS[sp["kind"]]
    S, U0, total, seed = sp["S"], sp["U0"], n_steps(sp["kind"]), sp["noise_seed"]
    state = np.random.get_state()
    try:
        if d["fam"] == "gp" and d["sampler"] == "rw":
            U, acc, _, _ = gcc.np_chains(sp["gp"]["c"], total, first_step=sp["base"], U0=U0, seed=SEED)
            return U, acc, None
        if d["fam"] == "gp":
            g = sp["gp"]
            args = (g["enka"], g["enka"].gpmodels, sp["y"], g["prior"], S, U0)
            if d["adapt"]:
                np.random.seed(seed)
                return _adapt_reference(sp, lambda S_: ac.gp_score(g["enka"], g["enka"].gpmodels, sp["y"], g["prior"], S_, d["mode"],
                                                                   sp["Gamma"], g["nugget"]))
            if d["sampler"] == "lv":
                U, rate = glc.np_chains_langevin(*args, total, d["mode"], sp["Gamma"], g["nugget"], seed)
            else:
                U, rate = hc.np_chains_hmc_gp(*args, total, d["L"], d["mode"], sp["Gamma"], g["nugget"], seed)
            return U, np.rint(rate * total).astype(np.int64), None
        if d["fam"] == "map":
            mk = sp["mapkind"]
            if d["adapt"]:
                np.random.seed(seed)
                return _adapt_reference(sp, lambda S_: ac.map_score(mk, S_))
            if d["sampler"] == "lv":
                U, acc = mlc.np_chains_mala(mk, S, U0, total, seed)
            else:
                U, acc = hc.np_chains_hmc(mk, S, U0, total, d["L"], seed)
            return U, acc, None
        lp = sp["lin"]
        if d["adapt"]:
            np.random.seed(seed)
            return _adapt_reference(sp, lambda S_: lhc.score_of(lp, S_))
        if d["sampler"] == "lv":
            U, acc = llc.np_chains_mala_lineal(lp, S, U0, total, seed)
        else:
            U, acc = lhc.np_chains(lp, S, U0, total, d["L"], seed)
        return U, acc, None
    finally:
        np.random.set_state(state)


def _adapt_reference(sp, score_of):
    """The adaptation phase (``np_adapt``), then the join as the sampler makes it -- the scales re-formed at delta * multiplier --
    and the POST_STEPS plain steps behind it (``hmc_cases._hmc_steps``, as ``adapt_cases.np_accept_rate`` runs them), the global
    RNG running on."""
    A, L = sp["adapt"], sp["L"]
    states, hist, mult, _ = ac.np_adapt(score_of(sp["S"]), sp["S"], sp["U0"], A, L, sp["target"])
    S2 = (sp["delta"] * mult) * sp["C"]
    with np.errstate(over="ignore", invalid="ignore"):
        U_end, acc = hc._hmc_steps(score_of(S2), S2, states[-1], POST_STEPS, L)
    return states[-1], acc, dict(history=hist, multiplier=mult, U_end=U_end)


# ---- the call-order table ----------------------------------------------------------------------------------------------------------
OK, EINVAL, ESTATE = "OK", "EINVAL", "ESTATE"

# The states a handle can be in, as attributes: kind the proposal ('rw' | 'lv' | None), start the LAST start, pending what is in
# flight ('lv': a cesx_*_langevin_propose, 'lin_lv', 'hmc': a cesx_mh_hmc_begin, 'lin_hmc'), armed / done the adaptation, lin a
# lineal image.  Everything that can be installed is: the problem, a GP image with n_gp = n_obs = k, the banana map, the proj descriptor.
def _row(kind=None, start=None, pending=None, armed=False, done=False, lin=False):
    return dict(kind=kind, start=start, pending=pending, armed=armed, done=done, lin=lin)


ROWS = {
    "no_proposal": _row(),
    "rw_unstarted": _row("rw"),
    "pcn_unstarted": _row("rw"),
    "mh_start": _row("rw", "mh"),
    "gp_start": _row("rw", "gp"),
    "gp_langevin_start": _row("lv", "gp_lv", lin=True),
    "mh_langevin_start": _row("lv", "mh_lv", lin=True),
    "lineal_start": _row("lv", "lin", lin=True),
    "proj_start": _row("lv", "proj", lin=True),
    "proposed": _row("lv", "mh_lv", "lv", lin=True),
    "lineal_proposed": _row("lv", "lin", "lin_lv", lin=True),
    "begun": _row("lv", "mh_lv", "hmc", lin=True),
    "lineal_begun": _row("lv", "lin", "lin_hmc", lin=True),
    "armed": _row("lv", "mh_lv", armed=True, lin=True),
    "lineal_armed": _row("lv", "lin", armed=True, lin=True),
    "armed_done": _row("lv", "mh_lv", armed=True, done=True, lin=True),
    "lineal_reinstalled": _row("lv", None, lin=True),
    "lineal_set_behind_a_proposal": _row("lv", "mh_lv", lin=True),      # mh_langevin_start, a propose, then the re-install: the start stands, the proposal is over
    "after_set_problem": _row(),
}

COLUMNS = (
    "cesx_mh_start", "cesx_mh_propose", "cesx_mh_accept", "cesx_mh_run_map",
    "cesx_gp_predict", "cesx_gp_start", "cesx_gp_accept", "cesx_gp_run", "cesx_gp_predict_grad",
    "cesx_mh_langevin_start", "cesx_mh_langevin_propose", "cesx_mh_langevin_accept", "cesx_mh_langevin_run_map",
    "cesx_gp_langevin_start", "cesx_gp_langevin_propose", "cesx_gp_langevin_accept",
    "cesx_gp_proj_langevin_start", "cesx_gp_proj_langevin_accept",
    "cesx_mh_langevin_lineal_start", "cesx_mh_langevin_lineal_propose", "cesx_mh_langevin_lineal_accept",
    "cesx_mh_hmc_begin", "cesx_mh_hmc_leap", "cesx_mh_hmc_accept", "cesx_gp_hmc_leap", "cesx_gp_hmc_accept",
    "cesx_gp_proj_hmc_leap", "cesx_gp_proj_hmc_accept", "cesx_mh_hmc_run_map",
    "cesx_mh_hmc_lineal_begin", "cesx_mh_hmc_lineal_leap", "cesx_mh_hmc_lineal_accept",
)

# The cells include/cesx.h left open, and the sentence each was decided from (NOTEBOOK.md repeats them; the header now says so).
UNDECIDED = {        # key: (the decision and the sentence it was taken from, the words of the header's paragraph that now state it)
    "rw_after_other_start": ("cesx_mh_accept / cesx_mh_run_map after cesx_gp_start and cesx_gp_accept / cesx_gp_run after cesx_mh_start: OK -- "
                             "'The start, the test, the device uniform, the counters and cesx_mh_stats are those of cesx_mh_start / "
                             "cesx_mh_accept', and cesx_gp_run names both starts", "One start serves both random-walk families"),
    "langevin_kind_without_start": ("the random-walk calls under CESX_MH_LANGEVIN before any start: CESX_EINVAL -- 'With this kind ... "
                                    "return CESX_EINVAL and launch nothing' carries no condition",
                                    "return CESX_EINVAL whether or not a Langevin start has run"),
    "langevin_across_families": ("cesx_mh_langevin_propose / _accept / _run_map after cesx_gp_langevin_start or cesx_gp_proj_langevin_start "
                                 "and cesx_gp_langevin_propose / _accept after cesx_mh_langevin_start: OK -- 'The proposal and the begin of a "
                                 "trajectory are cesx_gp_langevin_propose and cesx_mh_hmc_begin, which take no mode; steps of both families "
                                 "alternate on one handle', and cesx_mh_langevin_run_map names both starts",
                                 "cesx_mh_langevin_start, cesx_gp_langevin_start and cesx_gp_proj_langevin_start are ONE family"),
    "lineal_reinstall": ("after cesx_mh_langevin_lineal_set on a handle whose last start was cesx_mh_langevin_lineal_start every step, "
                         "cesx_mh_phi and cesx_mh_stats: CESX_ESTATE until a new start -- 'cesx_set_problem and cesx_mh_set_proposal drop "
                         "the images', and g of the chains belonged to the image that was replaced",
                         "whose LAST start was cesx_mh_langevin_lineal_start ends that start"),
    "lineal_set_behind_other_start": ("cesx_mh_langevin_lineal_set behind one of the other three starts: the start stands, a pending proposal or "
                                      "trajectory is over (row lineal_set_behind_a_proposal) -- the install replaces images the other family does "
                                      "not read, and resets what is in flight as cesx_mh_adapt_set does",
                                      "After one of the other three starts the start stands, and a pending proposal or trajectory is ended"),
    "starts_while_pending": ("a start while a proposal or a trajectory is pending: OK, it ends them -- 'since the start or the last accept'",
                             "A start is accepted while a proposal or a trajectory is pending and ends it"),
}


def expect(row, col):
    """The answer of ``col`` on a handle in state ``row`` when every argument is valid, from the prose of include/cesx.h."""
    r = ROWS[row]
    kind, start, pend, armed, done, lin = r["kind"], r["start"], r["pending"], r["armed"], r["done"], r["lin"]
    lv_started = start in ("gp_lv", "mh_lv", "proj")          # 'the LAST start' was one of the Jacobian / emulator family
    if col in ("cesx_gp_predict", "cesx_gp_predict_grad"):    # need cesx_gp_set alone
        return OK
    if col in ("cesx_mh_start", "cesx_mh_propose", "cesx_mh_accept", "cesx_mh_run_map", "cesx_gp_start", "cesx_gp_accept", "cesx_gp_run"):
        if kind is None:                                      # 'A later cesx_set_problem drops the proposal'
            return ESTATE
        if kind == "lv":                                      # 'With this kind ... return CESX_EINVAL and launch nothing'
            return EINVAL
        if col in ("cesx_mh_start", "cesx_mh_propose", "cesx_gp_start"):
            return OK
        return OK if start in ("mh", "gp") else ESTATE        # 'CESX_ESTATE without ... a start (cesx_gp_start / cesx_mh_start)'
    if kind != "lv":                                          # 'CESX_ESTATE without ... a proposal of kind CESX_MH_LANGEVIN'
        return ESTATE
    if col in ("cesx_mh_langevin_start", "cesx_gp_langevin_start", "cesx_gp_proj_langevin_start"):
        return OK                                             # 'The starts ... stay available' while armed
    if col.startswith("cesx_mh_langevin_lineal_"):
        if armed or not lin:                                  # 'While armed ... the cesx_mh_langevin_lineal_* family return CESX_ESTATE'
            return ESTATE
        if col.endswith("_start"):
            return OK
        if start != "lin":                                    # 'unless the LAST start was cesx_mh_langevin_lineal_start'
            return ESTATE
        return OK if col.endswith("_propose") or pend == "lin_lv" else ESTATE
    if col.startswith("cesx_mh_hmc_lineal_"):
        if not lin or start != "lin" or (armed and done):     # 'after n_steps accepts they return CESX_ESTATE'
            return ESTATE
        return OK if col.endswith("_begin") or pend == "lin_hmc" else ESTATE
    if col in ("cesx_mh_langevin_propose", "cesx_gp_langevin_propose", "cesx_mh_langevin_run_map", "cesx_mh_hmc_run_map",
               "cesx_mh_langevin_accept", "cesx_gp_langevin_accept", "cesx_gp_proj_langevin_accept"):
        if armed or not lv_started:                           # 'While armed, cesx_mh_hmc_run_map, every cesx_*_langevin_propose / _accept / _run_map ...'
            return ESTATE
        if col.endswith("_accept"):                           # 'accept also without a propose since the start or the last accept'
            return OK if pend == "lv" else ESTATE
        return OK
    # the leapfrog calls: cesx_mh_hmc_begin / _leap / _accept, cesx_gp_hmc_*, cesx_gp_proj_hmc_*
    if not lv_started or (armed and done):
        return ESTATE
    return OK if col == "cesx_mh_hmc_begin" or pend == "hmc" else ESTATE


CALL_ORDER = {row: {col: expect(row, col) for col in COLUMNS} for row in ROWS}


def header_entry_points():
    """{name: parameter text} of every prototype of include/cesx.h."""
    with open(os.path.join(ROOT, "include", "cesx.h")) as fh:
        text = fh.read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return {m.group(1): " ".join(m.group(2).split()) for m in re.finditer(r"\b(cesx_\w+)\s*\(([^;{}]*?)\)\s*;", text)}


def chain_entry_points():
    """The cesx_mh_* / cesx_gp_* (cesx_gp_proj_* among them) entry points that take chains: a state, proposal or position block."""
    return sorted(name for name, prm in header_entry_points().items()
                  if re.match(r"cesx_(mh|gp)_", name) and re.search(r"\b(U_dev|P_dev|Q_dev|X_dev)\b", prm))
