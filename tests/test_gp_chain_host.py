"""The fused chain kernel of MCMC.gp_mh(chains=) as far as it goes without a GPU: cesx_gp_run in the header, the binding and the
cross-compiled library; the refusals of ``fused=True`` before any engine exists; the launch planner ``sample.fused_chunks``;
and gp_chain_kernel's rows of the register and scratch table (tools/isa_audit.py, recorded in
profiles/gp_chain_isa_audit.txt)."""
import itertools
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from test_emulate_host import gold_prior, gold_problem, load_gold  # noqa: E402
import gp_chain_cases as gc  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    from ces_amd import build, engine
    build.build_lib()
    return engine.load_library()


def test_abi_of_the_fused_gp_sampler(lib):
    from ces_amd import build, engine
    with open(os.path.join(ROOT, "include", "cesx.h")) as fh:
        hdr = fh.read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bint\s+cesx_gp_run\s*\(\s*cesx_handle h, int mode, uint64_t step_index, int n_steps, int stride, "
                     r"int nugget,", code)
    assert "cesx_gp_run" in engine.EXPORTS and hasattr(lib, "cesx_gp_run")
    assert "#define CESX_ABI_VERSION %d" % engine.ABI_VERSION in code and engine.ABI_VERSION >= 7
    assert lib.cesx_abi_version() == engine.ABI_VERSION
    assert "kernels_gpchain.hip" in build.SOURCES
    assert len(lib.cesx_gp_run.argtypes) == 11
    # a NULL handle: the error code, no device touched
    assert lib.cesx_gp_run(None, engine.GP_MODES["var"], 0, 1, 1, 1, None, None, None, None, None) == engine.EINVAL
    # the LDS limit is in the header as a formula
    assert "256 (3 p + J_p + 2 n_gp) + 8192 bytes <= 160 KiB" in hdr


def test_fused_refusals_come_before_any_engine():
    from ces_amd import sample
    man, a = load_gold()
    enka = gold_problem(a)
    mc = sample.MCMC()
    mc.mute_bar, mc.y_obs = True, a["prob_y"]
    assert sample.MCMC.GP_FUSED_DEFAULT is False
    pca = dict(VD_k=a["prob_VD_k"], mG=a["prob_mG"])
    with pytest.raises(ValueError, match="fused"):                        # without chains=
        mc.gp_mh(enka, 2, gold_prior(a), fused=True)
    with pytest.raises(ValueError, match="fused.*pca_tools"):             # mode dense
        mc.gp_mh(enka, 2, gold_prior(a), chains=4, fused=True, pca_tools=pca, Gamma=a["prob_Gamma_dense"])
    with pytest.raises(ValueError, match="fused.*pca_tools"):             # mode projected
        mc.gp_mh(enka, 2, gold_prior(a), chains=4, fused=True, pca_tools=pca, Gamma=a["prob_Gamma_dense"],
                 sigma_form="projected")
    with pytest.raises(ValueError, match="fused.*separable"):
        mc.gp_mh(enka, 2, gold_prior(a), chains=4, fused=True, separable=True)
    with pytest.raises(ValueError, match="fused must be"):
        mc.gp_mh(enka, 2, gold_prior(a), chains=4, fused="yes")
    assert not hasattr(mc, "_mh_eng") and not hasattr(mc, "samples")


def test_gp_fused_work_is_fifty_steps_at_e1():
    """The derivation next to the constant: shape E1 (65 536 chains, p = 8, 32 GPs, J_t = 512) gets 50 steps per launch."""
    from ces_amd import sample
    M, p, n_gp, Jp = 65536, 8, 32, 512
    work = M * n_gp * Jp * (Jp // 2 + p + 8)
    # (the trace of every 100th step: the buffer budget alone would allow 1 600 steps)
    K_max, chunks = sample.fused_chunks(1000, 100, sample.MCMC.FUSED_STEPS_MAX, sample.MCMC.FUSED_BUFFER_BYTES, M * p * 8 // 100,
                                        sample.MCMC.GP_FUSED_WORK, work)
    assert K_max == 100 and chunks == [100] * 10             # a stride over the cap: one stride per launch
    K_max, chunks = sample.fused_chunks(1000, 10, sample.MCMC.FUSED_STEPS_MAX, sample.MCMC.FUSED_BUFFER_BYTES, M * p * 8 // 10,
                                        sample.MCMC.GP_FUSED_WORK, work)
    assert K_max == 50 and chunks == [50] * 20
    # a notebook shape (1 024 chains, p = 2, 2 GPs, J_t = 50) is capped by FUSED_STEPS_MAX, not by the work
    work = 1024 * 2 * 64 * (32 + 2 + 8)
    K_max, chunks = sample.fused_chunks(10000, 1, sample.MCMC.FUSED_STEPS_MAX, sample.MCMC.FUSED_BUFFER_BYTES, 1024 * 2 * 8,
                                        sample.MCMC.GP_FUSED_WORK, work)
    assert K_max == 4096 and chunks == [4096, 4096, 1808]


def test_chunk_planner():
    """Across stride, the step cap, the buffer budget and the work cap: every launch is a multiple of the stride (but the
    run's last), the launches sum to n_mcmc, and none is over a cap -- except that a stride longer than every cap makes
    launches of one stride, the shortest that keeps the kept states aligned."""
    from ces_amd import sample
    cases = itertools.product((0, 1, 7, 100, 1000, 4097), (1, 3, 100, 5000), (1, 64, 4096), (1 << 10, 1 << 20),
                              (8, 4096, 1 << 19), (None, 1000, 10 ** 6), (1, 999, 10 ** 5))
    n_cases = 0
    for n_mcmc, stride, steps_max, budget, per_step, work_max, work in cases:
        K_max, chunks = sample.fused_chunks(n_mcmc, stride, steps_max, budget, per_step, work_max, work)
        cap = min(steps_max, budget // per_step)
        if work_max is not None:
            cap = min(cap, work_max // work)
        cap = max(cap, 1)
        case = (n_mcmc, stride, steps_max, budget, per_step, work_max, work)
        assert sum(chunks) == n_mcmc and all(K >= 1 for K in chunks), case
        assert K_max % stride == 0 and K_max >= stride, case
        assert all(K == K_max for K in chunks[:-1]) and all(K <= K_max for K in chunks), case
        assert all(K % stride == 0 for K in chunks[:-1]), case
        assert K_max <= cap or K_max == stride, case
        if stride <= cap:
            assert K_max > cap - stride, case                  # as long as the caps allow
        n_cases += 1
    assert n_cases == 6 * 4 * 3 * 2 * 3 * 3 * 3
    # no work cap without a work figure (model_mh)
    assert sample.fused_chunks(10, 1, 4096, 1 << 26, 16, None, 0) == (4096, [10])
    assert sample.fused_chunks(10, 1, 4096, 1 << 26, 16, 5, 0) == (4096, [10])


@pytest.fixture(scope="module")
def table():
    import isa_audit
    t = isa_audit.collect(["kernels_gpchain.hip"])
    names = isa_audit.demangle(sorted(t))
    return {re.sub(r"\(.*", "", names[k]).replace("cesx::", "").replace("void ", ""): v for k, v in t.items()}


def test_the_gp_chain_kernels_have_no_scratch_and_no_spills_in_the_loop(table):
    rows = {k: v for k, v in table.items() if k.startswith("gp_chain_kernel<")}
    assert sorted(rows) == ["gp_chain_kernel<double>", "gp_chain_kernel<float>"]
    for name, r in rows.items():
        assert r["ScratchSize [bytes/lane]"] == 0 and r["scratch_total"] == 0, name
        assert r["VGPRs Spill"] == 0 and r["spill_in_loop"] == 0, name
        assert r["mfma_in_loop"] > 0, name
    # the file holds no kernel that tests/test_emulate_host.py counts in kernels_gp.hip
    assert not any("gp_predict_kernel" in k or "gp_score_kernel" in k for k in table)


def test_the_cases_cover_every_value():
    cs = gc.cases()
    assert len(cs) == 20 and len({gc.case_id(c) for c in cs}) == 20
    for key, want in (("M", {1, 31, 32, 33, 65}), ("Jt", {15, 16, 17, 33}), ("p", {1, 2, 5}), ("n", {1, 4}),
                      ("family", set(gc.FAMILIES)), ("nugget", {False, True}),
                      ("mode", {"gamma", "gamma_dense", "var", "gamma_var"}), ("prior", {"rw_dense", "pcn", "rw_diag"})):
        assert {c[key] for c in cs} == want, key
    assert {(c["M"], c["Jt"]) for c in cs} == set(itertools.product((1, 31, 32, 33, 65), (15, 16, 17, 33)))


@pytest.mark.parametrize("c", gc.cases(), ids=gc.case_id)
def test_no_decision_of_a_case_sits_within_rounding_of_the_test(c):
    """The device comparison of the fused kernel with the step path asks for EQUAL accept counters of every chain.  That holds
    when no decision has log u within rounding of phi(U) - phi(P): here the fp64 numpy chains under the device noise, over the
    12 steps the device test covers (7 from step 0; 5 + 7 through the resume), keep every decision 1e-7 away from its
    threshold -- 1e6 times the error either path makes in phi -- and both accept and reject."""
    U, acc, margin, _ = gc.np_chains(c, 12)
    print("\n[gp chain] %s: margin %.3g, accepted %d of %d" % (gc.case_id(c), margin, acc.sum(), 12 * c["M"]))
    assert margin > 1e-7
    if c["M"] >= 31:
        assert 0 < acc.sum() < 12 * c["M"]
