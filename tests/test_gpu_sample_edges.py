"""The Sample stage at its ragged and strided edges (kernels_mh.hip; the proposal's update launches; the device uniform).

mh_accept_kernel is driven directly with arrays made here -- U, P, G(U), G(P) rounded to the engine dtype on the host --
and compared, step by step, with the fp64 reference of oracle/stage_ref.py computed FROM THOSE ROUNDED VALUES: what is
left between the two is the order of an fp64 sum.  A chain-step is left out of the comparison when it is a tie,
|phi(U) - phi(P) - log u| <= 1e-9 max(1, |phi(U)|) (1e-9: the bar the project holds fp64 paths to); the reference then
adopts the device's decision for that chain and goes on, so a tie costs one chain-step and not the chain.  At most 1
chain-step in 1000 may be left out per case (asserted).  Everywhere else the device's U must equal where(accept, P, U)
bit for bit, the per-chain counters must equal the reference's, and the guard elements around U must be untouched.

RW with a dense Sigma in fp32 is the one case whose inputs are not all the test's own: w = L_Sigma^{-1} (x - mu) comes
from a triangular update launch in fp32.  Its band comes from the reference alone: w in fp64, rounded to fp32, the
largest |phi(w rounded) - phi(w)| over the chains, times 10 (the launch sums p terms in fp32, not one rounding).

The device uniform (logu=None) is compared with its restatement in oracle/stage_ref.py under the same band, and the
proposal with noise drawn on the device with a U + b S noise_block(...) under the ensemble bars of DESIGN.md section 6."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import rel_err  # noqa: E402
from edge_helpers import guarded, guards_intact, put, same_bits  # noqa: E402,F401
from test_gpu_mcmc import _problem  # noqa: E402

from oracle import stage_ref as sr  # noqa: E402

pytestmark = pytest.mark.gpu

STEPS = 20
ENSEMBLE_BAR = {"float64": 1e-6, "float32": 1e-3}
WORST = {}                       # per part: chain-steps left out, chain-steps, worst ratio of an error to its bar


@pytest.fixture(scope="module")
def eng_mod():
    import torch
    from ces_amd import engine
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return engine


def note(part, ref=None, ratio=None):
    w = WORST.setdefault(part, {"left_out": 0, "chain_steps": 0, "ratio": 0.0})
    if ref is not None:
        w["left_out"] += ref.left_out
        w["chain_steps"] += ref.chain_steps
    if ratio is not None:
        w["ratio"] = max(w["ratio"], ratio)
    return w


def run_accept_steps(eng, U_flat, U, Uh, ref, step_ids, make_step, launch, label, part):
    """The comparison loop of the accept kernels.  make_step(k, Uh) -> dict with P (engine dtype, host), phi_p, logu
    (host, fp64), optionally half_width; launch(step_index, d) runs the device's accept step on U."""
    M = eng.J
    taken_total = 0
    for k, step in enumerate(step_ids):
        d = make_step(k, Uh)
        launch(step, d)
        Un = U.cpu().numpy()
        acc, band = ref.decide(d["phi_p"], d["logu"], d.get("half_width"))
        took = np.all(same_bits(Un, d["P"]), axis=0)
        kept = np.all(same_bits(Un, Uh), axis=0)
        assert np.all(took | kept), (label, k, "a column is neither the proposal nor the old state",
                                     np.flatnonzero(~(took | kept))[:8])
        ok = ~band
        want = np.where(acc[None, :], d["P"], Uh)
        bad = ok & ~np.all(same_bits(Un, want), axis=0)
        assert not bad.any(), (label, "step %d" % k, "chains", np.flatnonzero(bad)[:8], "of", int(bad.sum()))
        taken = np.where(band, took & ~kept, acc)
        ref.commit(taken, d["phi_p"], band)
        nsteps, rate, per = eng.mh_stats(per_chain=True)
        assert nsteps == k + 1
        assert np.array_equal(per.astype(np.int64), ref.count), (label, k, np.flatnonzero(per.astype(np.int64) != ref.count)[:8])
        assert rate == pytest.approx(ref.count.sum() / ((k + 1) * M), abs=1e-12)
        assert guards_intact(U_flat, U), (label, k, "written outside U")
        taken_total += int(taken.sum())
        Uh = Un
    w = note(part, ref)
    print("%s: %d of %d chain-steps left out (cap %d), %d accepted; %s so far %d of %d"
          % (label, ref.left_out, ref.chain_steps, ref.chain_steps // 1000, taken_total, part, w["left_out"], w["chain_steps"]))
    assert ref.within_cap(), (label, ref.left_out, ref.chain_steps)
    return Uh, taken_total


def mh_case(eng_mod, dtype, p, n, M, kind, dense=False, shift=0, uniform=None, part="A"):
    """One case of mh_accept_kernel.  kind None (RW) or 'pCN'; dense: a dense Sigma (RW); shift: the buffers start that
    many elements off 16-byte alignment; uniform (seed, j_offset, step indices): the device's own log u."""
    import torch
    ndt = np.dtype(dtype)
    rng = np.random.default_rng([p, n, M, 1 if dtype == "float32" else 0, 1 if kind else 0, 1 if dense else 0, shift])
    A, y, Gamma, mu, Sigma = _problem(rng, p, n, dense_sigma=dense)
    S = np.sqrt(0.3 / n) * np.linalg.cholesky(Sigma)
    beta = 0.3
    gw = 1.0 / np.diag(Gamma)
    kw, step_ids = {}, list(range(STEPS))
    if uniform is not None:
        seed, j_offset, step_ids = uniform
        kw = dict(seed=seed, j_offset=j_offset, J_global=j_offset + M)
    eng = eng_mod.Engine(p, n, M, dtype=dtype, **kw)
    if kind == "pCN":
        # pCN has no prior rows: a prior the reference never sees must not move a decision
        Bd = rng.standard_normal((p, p)) / np.sqrt(p)
        eng.set_problem(y, Gamma, mu + 100.0, 0.5 * (Bd @ Bd.T) + 0.5 * np.eye(p), mu)
    else:
        eng.set_problem(y, Gamma, mu, Sigma, mu)
    eng.mh_set_proposal(kind, S, beta)

    def f64(a):
        return a.astype(np.float64)

    def phi_and_hw(Xh, Gh):
        """the reference's phi of the rounded values; for the fp32 dense prior also max |phi(w rounded) - phi(w)|"""
        if kind == "pCN":
            return sr.mh_phi(f64(Gh), y, gw), 0.0
        if not dense:
            return sr.mh_phi(f64(Gh), y, gw, f64(Xh), mu, 1.0 / np.diag(Sigma)), 0.0
        w = sr.dense_prior_rows(f64(Xh), mu, Sigma)
        ph = sr.mh_phi(f64(Gh), y, gw, w)
        return ph, float(np.max(np.abs(sr.mh_phi(f64(Gh), y, gw, f64(w.astype(ndt))) - ph)))

    U_flat, U = guarded(eng, p, shift)
    G_flat, G = guarded(eng, n, shift)
    P_flat, P = guarded(eng, p, shift)
    GP_flat, GP = guarded(eng, n, shift)
    Uh = (mu[:, None] + 0.3 * rng.standard_normal((p, M))).astype(ndt)
    Gh = (A @ f64(Uh)).astype(ndt)
    put(U, Uh)
    put(G, Gh)
    eng.mh_start(U, G)
    assert np.all(same_bits(U.cpu().numpy(), Uh)) and guards_intact(U_flat, U)
    ph0, hw0 = phi_and_hw(Uh, Gh)
    ref = sr.AcceptRef(ph0)
    own_band = dense and dtype == "float32"
    state = {"hw": hw0}

    def make_step(k, Uh):
        Ph = sr.propose(f64(Uh), S, rng.standard_normal((p, M)), kind, beta).astype(ndt)
        GPh = (A @ f64(Ph)).astype(ndt)
        phi_p, hw = phi_and_hw(Ph, GPh)
        state["hw"] = max(state["hw"], hw)
        logu = np.log(rng.random(M)) if uniform is None else sr.log_uniform(M, seed, step_ids[k], j_offset)
        d = dict(P=Ph, GP=GPh, phi_p=phi_p, logu=logu)
        if own_band:
            d["half_width"] = 10.0 * state["hw"]
        return d

    def launch(step, d):
        put(P, d["P"])
        put(GP, d["GP"])
        lu = None if uniform is not None else torch.as_tensor(d["logu"], dtype=torch.float64, device=eng.device)
        eng.mh_accept(step, U, P, GP, logu=lu)
        assert np.all(same_bits(P.cpu().numpy(), d["P"])) and np.all(same_bits(GP.cpu().numpy(), d["GP"]))

    label = "mh_accept %s p=%d n=%d M=%d %s%s%s%s" % (dtype, p, n, M, kind or "RW", " dense Sigma" if dense else "",
                                                       " unaligned" if shift else "",
                                                       " device uniform j_offset=%d" % uniform[1] if uniform else "")
    Uh, taken = run_accept_steps(eng, U_flat, U, Uh, ref, step_ids, make_step, launch, label, part)
    for flat, view in ((G_flat, G), (P_flat, P), (GP_flat, GP)):
        assert guards_intact(flat, view)
    if own_band:
        print("%s: half-width %.3e at |phi| ~ %.3g, share left out %.2e"
              % (label, 10.0 * state["hw"], float(np.median(np.abs(ref.phi))), ref.left_out / ref.chain_steps))
    if M >= 63:                        # (both branches of the copy ran: some chains moved, some did not)
        assert 0 < taken < len(step_ids) * M, (label, taken)
    return ref


# ---- A. mh_accept_kernel against the fp64 reference of the same inputs -----------------------------------------------

RAGGED_M = [1, 2, 3, 5, 63, 130, 255, 257, 1023, 4099]
ROW_SHAPES = [(1, 1), (15, 17), (16, 16), (33, 100), (64, 64), (256, 256)]


@pytest.mark.parametrize("kind", [None, "pCN"], ids=["RW", "pCN"])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("M", RAGGED_M)
def test_accept_ragged_chain_counts(eng_mod, M, dtype, kind):
    """Chain counts that are not multiples of the loads' width nor of a workgroup (256 / 128 chains): the scalar loads,
    the partly filled last workgroup and the element-wise copy of accepted columns."""
    mh_case(eng_mod, dtype, 5, 3, M, kind)


@pytest.mark.parametrize("kind", [None, "pCN"], ids=["RW", "pCN"])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("M", [1023, 1028])
@pytest.mark.parametrize("p,n", ROW_SHAPES)
def test_accept_row_counts_over_the_waves(eng_mod, p, n, M, dtype, kind):
    """Rows split over the 16 waves of a workgroup: fewer rows than waves, one short of / exactly / past a round of
    them, and many rounds; M = 1023 (scalar loads) and 1028 (16-byte loads, the last workgroup partly filled)."""
    mh_case(eng_mod, dtype, p, n, M, kind)


@pytest.mark.parametrize("kind", [None, "pCN"], ids=["RW", "pCN"])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_accept_from_unaligned_views(eng_mod, dtype, kind):
    """M a multiple of 4, every buffer one element off 16-byte alignment: the alignment test picks the scalar loads."""
    mh_case(eng_mod, dtype, 33, 100, 1028, kind, shift=1)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("M", [1023, 1024])
@pytest.mark.parametrize("p,n", [(33, 100), (64, 64)])
def test_accept_with_a_dense_prior(eng_mod, p, n, M, dtype):
    mh_case(eng_mod, dtype, p, n, M, None, dense=True, part="A dense Sigma " + dtype)


# ---- B. the device uniform and the MH noise domain against oracle/philox.py ------------------------------------------

SEED = 0x9E3779B97F4A7C15            # a non-zero high word
UNIFORM_STEPS = [0, 1] + list(range(2, STEPS - 1)) + [2 ** 31 - 1]


@pytest.mark.parametrize("kind", [None, "pCN"], ids=["RW", "pCN"])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("j_offset", [0, 2 ** 32 + 7])
@pytest.mark.parametrize("M", [5, 1023, 4099])
def test_accept_with_the_device_uniform(eng_mod, M, j_offset, dtype, kind):
    assert len(UNIFORM_STEPS) == STEPS and {0, 1, 2 ** 31 - 1} <= set(UNIFORM_STEPS)
    mh_case(eng_mod, dtype, 5, 3, M, kind, uniform=(SEED, j_offset, UNIFORM_STEPS), part="B uniform")


# One shape per branch of pick_update_kernel (kernels_update.hip), by its documented conditions: M % 4 == 0 and aligned
# buffers take the LDS-DMA kernels -- p <= 64 the LDS-resident small kernels (update2s fp32, update3s fp64), larger p
# update2 / update3 -- and M % 4 != 0 the register-staged update_kernel.  fp32 draws xi inside the update kernel, fp64
# through the noise kernel into the engine's buffer.  Nothing here asserts which kernel ran.
PROPOSE_SHAPES = [(33, 1024), (256, 1024), (33, 1023), (256, 1023)]


@pytest.mark.parametrize("kind", [None, "pCN"], ids=["RW", "pCN"])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("p,M", PROPOSE_SHAPES)
def test_propose_with_device_noise(eng_mod, p, M, dtype, kind):
    ndt = np.dtype(dtype)
    rng = np.random.default_rng([p, M, 1 if kind else 0])
    beta = 0.3
    B = rng.standard_normal((p, p)) / np.sqrt(p)
    S = np.linalg.cholesky(0.5 * (B @ B.T) + 0.5 * np.eye(p))
    for j_offset, step in ((0, 0), (0, 3), (2 ** 32 + 7, 2 ** 31 - 1)):
        eng = eng_mod.Engine(p, 2, M, dtype=dtype, seed=SEED, j_offset=j_offset, J_global=j_offset + M)
        eng.set_problem(np.zeros(2), np.eye(2), np.zeros(p), np.eye(p), np.zeros(p))
        eng.mh_set_proposal(kind, S, beta)
        Uh = rng.standard_normal((p, M)).astype(ndt)
        U_flat, U = guarded(eng, p)
        P_flat, P = guarded(eng, p)
        put(U, Uh)
        eng.mh_propose(step, U, out=P)
        got = P.cpu().numpy()
        xi = sr.mh_noise(p, M, SEED, step, j_offset, ndt)
        want = sr.propose(Uh.astype(np.float64), S, xi, kind, beta)
        err = rel_err(got, want)
        w = note("B propose " + dtype, ratio=err / ENSEMBLE_BAR[dtype])
        print("mh_propose %s p=%d M=%d %s j_offset=%d step=%d: rel err %.3e (bar %.0e, ratio %.3g; worst so far %.3g)"
              % (dtype, p, M, kind or "RW", j_offset, step, err, ENSEMBLE_BAR[dtype], err / ENSEMBLE_BAR[dtype], w["ratio"]))
        assert err <= ENSEMBLE_BAR[dtype], (j_offset, step, err)
        assert np.all(same_bits(U.cpu().numpy(), Uh)) and guards_intact(U_flat, U) and guards_intact(P_flat, P)
        # the EKS domain of the same step index is another block
        assert rel_err(got, sr.propose(Uh.astype(np.float64), S,
                                       sr.noise_block(p, M, SEED, step, j_offset, ndt), kind, beta)) > 0.1
