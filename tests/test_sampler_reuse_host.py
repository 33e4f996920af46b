"""The tables of tests/sampler_reuse_cases.py, without a device: the generated sequences cover every ordered pair of block kinds,
the call-order table has a column for every chain-taking entry point of include/cesx.h, the fp32 tables reflect what the header
refuses on an fp32 engine, the problems of a kind differ as they are meant to, and the comparator sees a one-ulp change."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampler_reuse_cases as sc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    with open(os.path.join(ROOT, "include", "cesx.h")) as fh:
        return fh.read()


def test_block_kinds_per_engine():
    need = {"rw", "pcn", "rw_fused", "gp_gamma", "gp_var", "gp_gamma_var", "gp_dense", "gp_proj", "gp_run", "gp_lv", "gp_hmc",
            "gp_proj_lv", "gp_proj_hmc", "map_lv", "map_lv_fused", "map_hmc", "map_hmc_fused", "lin_lv", "log_lv", "lin_hmc",
            "adapt_map", "adapt_gp", "adapt_lin"}
    assert set(sc.kinds_of("A")) == need
    maps = {"rw_fused", "map_lv", "map_lv_fused", "map_hmc", "map_hmc_fused", "adapt_map"}       # need p = n_obs = 2
    assert set(sc.kinds_of("B")) == need - maps
    assert sc.ENGINES["A"] == dict(p=2, n=2, J=130, k=2) and sc.ENGINES["B"] == dict(p=3, n=5, J=257, k=3)
    for k in ("gp_hmc", "gp_proj_hmc", "map_hmc", "map_hmc_fused", "lin_hmc", "adapt_map"):
        assert sc.KINDS[k]["L"] == 3
    assert sc.STEPS == 3 and sc.A_STEPS == 3 and sc.POST_STEPS == 2


@pytest.mark.parametrize("dtype", sc.DTYPES)
@pytest.mark.parametrize("E", sorted(sc.ENGINES))
def test_pair_cover(E, dtype):
    """Every ordered pair (X, Y) of the kinds the engine hosts is consecutive in some part of the cover, X = X included, and then
    on the other problem."""
    kinds = sc.kinds_of(E, dtype)
    got = set()
    for X in kinds:
        seq = sc.pair_cover(E, dtype, X)
        assert seq[0][0] == X
        got |= sc.pairs_in(seq)
        same = [(a, b) for a, b in zip(seq, seq[1:]) if a[0] == b[0] == X]
        assert same and all(a[1] != b[1] for a, b in same)                     # X behind X: the other problem
        for a, b in zip(seq, seq[1:]):                                         # consecutive blocks never share numbers
            assert (a[0], a[1]) != (b[0], b[1])
        assert {it[2] for it in seq} == set(sc.NOISES) and all(it[3] is None for it in seq)
    assert got == {(a, b) for a in kinds for b in kinds}
    print("\n[pair cover] engine %s %s: %d kinds, %d ordered pairs, %d blocks" % (E, dtype, len(kinds), len(got),
                                                                                sum(len(sc.pair_cover(E, dtype, X)) for X in kinds)))


@pytest.mark.parametrize("E", sorted(sc.ENGINES))
def test_polluters_and_abandoned_work_stand_in_front_of_every_kind(E):
    kinds = set(sc.kinds_of(E))
    pol = sc.polluters(E)
    assert pol and all(sc.gradient(k) and not sc.KINDS[k]["fused"] for k in pol)
    assert set(pol) == {k for k in kinds if sc.gradient(k)} - {"map_lv_fused", "map_hmc_fused"}
    for X in pol:
        seq = sc.nan_cover(E, "float64", X)
        assert {b[0] for a, b in zip(seq, seq[1:]) if a[3] == "nan"} == kinds
        assert all(a[0] == X for a in seq if a[3] == "nan")
    for form in sc.ABANDON_FORMS:
        who = sc.abandoners(E, "float64", form)
        seq = sc.abandon_cover(E, "float64", form)
        assert who and {b[0] for a, b in zip(seq, seq[1:]) if a[3] == form} == kinds
        assert {a[0] for a in seq if a[3] == form} == set(who)                 # every kind the form fits is interrupted once
    assert all(sc.KINDS[k]["sampler"] == "hmc" for k in sc.abandoners(E, "float64", "ab_leap"))
    assert all(sc.KINDS[k]["adapt"] for k in sc.abandoners(E, "float64", "ab_adapt"))


def test_fp32_refusals_are_the_headers():
    """The fp32 tables are the fp64 ones less the blocks the header refuses on an fp32 engine.  It refuses none in the Sample and
    Emulate stages: no sentence between the Sample stage's heading and the GP training says so, and the table is empty."""
    text = _header()
    a, b = text.index("MCMC.model_mh (ces/sample.py"), text.index("---- Emulate: training the GPs on device")
    assert 0 < a < b
    # every sentence there that names an engine dtype next to any word of refusal (an error code, 'refuse', 'unsupported',
    # 'cannot', 'only on an fp64 engine', ...) has to be accounted for by the table: a kind removed, with that sentence
    hits = sc.fp32_refusal_sentences(text[a:b])
    assert sorted(hits) == sorted(sc.FP32_REFUSED.values()), hits
    assert sum(1 for _ in sc.FP32_ENGINE_WORDS.finditer(text[a:b])) >= 20        # (the search does read the dtype sentences)
    planted = text[a:b] + " /* On an fp32 engine cesx_mh_hmc_lineal_begin returns CESX_EUNSUPPORTED. */"
    assert len(sc.fp32_refusal_sentences(planted)) == 1 and len(sc.fp32_refusal_sentences(text[a:b] + " /* fp64 engines only. */")) == 1
    for E in sc.ENGINES:
        assert sc.kinds_of(E, "float32") == [k for k in sc.kinds_of(E, "float64") if k not in sc.FP32_REFUSED]
    # what the header does say of an fp32 engine there: it rounds where it stores
    assert "an fp32 engine rounds where it stores" in text[a:b]


@pytest.mark.parametrize("E", sorted(sc.ENGINES))
def test_two_problems_per_block(E):
    """The two problems of a kind differ in y, the prior, the start states' scale and -- unless the kind needs one form -- in
    whether Gamma is dense; step indices and injected draws are the block's own."""
    one_form = {"gp_var", "gp_gamma_var", "gp_lv", "adapt_gp"}                 # diag(gvars) needs a diagonal Gamma
    bases = set()
    for kind in sc.kinds_of(E):
        a, b = sc.spec(E, kind, 0), sc.spec(E, kind, 1)
        e = sc.ENGINES[E]
        for s in (a, b):
            assert s["U0"].shape == (e["p"], e["J"]) and s["S"].shape == (e["p"], e["p"]) and np.all(np.triu(s["S"], 1) == 0)
            assert s["y"].shape == (e["n"],) and s["Gamma"].shape == (e["n"], e["n"]) and np.all(np.isfinite(s["U0"]))
            assert len({tuple(c) for c in s["U0"].T}) == e["J"]                # every chain starts somewhere else
        assert not np.array_equal(a["y"], b["y"]) and not np.array_equal(a["cov"], b["cov"])        # the data and the prior
        dense = [bool(np.any(s["Gamma"] != np.diag(np.diag(s["Gamma"])))) for s in (a, b)]
        if kind in one_form:
            assert dense == [False, False]
        else:
            assert sorted(dense) == [False, True], (kind, dense)
        assert (a["spread"], b["spread"]) == (1.0, 0.4)                        # the start states about their centre
        assert a["base"] != b["base"] and a["noise_seed"] != b["noise_seed"]
        bases |= {a["base"], b["base"]}
        xi, lu = sc.injected(a)
        assert xi.shape == (sc.n_steps(kind), e["p"], e["J"]) and lu.shape == (sc.n_steps(kind), e["J"]) and np.all(lu < 0)
    assert len(bases) == 2 * len(sc.kinds_of(E))
    if E == "A":
        assert sc.spec("A", "rw", 0)["cov"][0, 1] != 0 and sc.spec("A", "pcn", 1)["cov"][0, 1] != 0       # rw and pcn: a dense prior
    else:
        assert sc.spec("B", "rw", 0)["cov"][0, 1] != 0 and sc.spec("B", "pcn", 1)["cov"][0, 1] != 0


def test_call_order_table_is_complete_against_the_header():
    """Every cesx_mh_* / cesx_gp_* / cesx_gp_proj_* entry point of include/cesx.h that takes chains is a column: a new entry
    point fails here until it has been placed in the table."""
    names = sc.chain_entry_points()
    assert len(names) >= 32 and "cesx_gp_proj_hmc_accept" in names and "cesx_mh_hmc_lineal_leap" in names
    assert sorted(sc.COLUMNS) == names, (sorted(set(names) - set(sc.COLUMNS)), sorted(set(sc.COLUMNS) - set(names)))
    assert len(set(sc.COLUMNS)) == len(sc.COLUMNS)
    for row in sc.ROWS:
        assert set(sc.CALL_ORDER[row]) == set(sc.COLUMNS)
        assert set(sc.CALL_ORDER[row].values()) <= {sc.OK, sc.EINVAL, sc.ESTATE}
    # the installs and reads that take no chains are not columns
    for name in ("cesx_mh_set_proposal", "cesx_mh_langevin_lineal_set", "cesx_mh_langevin_lineal_g", "cesx_gp_set", "cesx_gp_proj_coef",
                 "cesx_mh_adapt_set", "cesx_mh_adapt_read", "cesx_mh_stats", "cesx_mh_phi"):
        assert name in sc.header_entry_points() and name not in names


def test_call_order_rows_and_known_cells():
    need = {"no_proposal", "rw_unstarted", "pcn_unstarted", "mh_start", "gp_start", "gp_langevin_start", "mh_langevin_start", "lineal_start",
            "proj_start", "proposed", "begun", "armed", "armed_done", "lineal_reinstalled", "after_set_problem"}
    assert need <= set(sc.ROWS)
    T = sc.CALL_ORDER
    # sentences of the header, cell by cell
    assert T["mh_langevin_start"]["cesx_mh_accept"] == sc.EINVAL            # 'With this kind ... return CESX_EINVAL'
    assert T["rw_unstarted"]["cesx_mh_accept"] == sc.ESTATE and T["rw_unstarted"]["cesx_mh_propose"] == sc.OK
    assert T["mh_start"]["cesx_mh_langevin_propose"] == sc.ESTATE           # 'a proposal of kind CESX_MH_LANGEVIN'
    assert T["lineal_start"]["cesx_mh_langevin_propose"] == sc.ESTATE       # 'after a cesx_mh_langevin_lineal_start ... CESX_ESTATE until a start of their own'
    assert T["mh_langevin_start"]["cesx_mh_langevin_lineal_propose"] == sc.ESTATE       # 'and the other way round'
    assert T["mh_langevin_start"]["cesx_mh_langevin_accept"] == sc.ESTATE   # 'accept also without a propose'
    assert T["proposed"]["cesx_mh_langevin_accept"] == sc.OK and T["proposed"]["cesx_mh_hmc_leap"] == sc.ESTATE
    assert T["begun"]["cesx_mh_langevin_accept"] == sc.ESTATE               # 'It ends a pending cesx_*_langevin_propose, as such a propose ends a trajectory'
    assert T["begun"]["cesx_mh_hmc_accept"] == sc.OK and T["begun"]["cesx_gp_hmc_leap"] == sc.OK
    assert T["lineal_start"]["cesx_mh_hmc_begin"] == sc.ESTATE              # 'not cesx_mh_langevin_lineal_start: the linear maps have cesx_mh_hmc_lineal_*'
    assert T["armed"]["cesx_mh_hmc_begin"] == sc.OK and T["armed"]["cesx_mh_hmc_run_map"] == sc.ESTATE
    assert T["armed"]["cesx_mh_langevin_propose"] == sc.ESTATE and T["armed"]["cesx_mh_langevin_lineal_start"] == sc.ESTATE
    assert T["armed"]["cesx_mh_langevin_start"] == sc.OK                    # 'The starts ... stay available'
    assert T["lineal_armed"]["cesx_mh_hmc_lineal_begin"] == sc.OK           # 'cesx_mh_hmc_lineal_* is their armed form'
    assert T["armed_done"]["cesx_mh_hmc_begin"] == sc.ESTATE                # 'after n_steps accepts they return CESX_ESTATE'
    assert T["after_set_problem"]["cesx_gp_predict"] == sc.OK               # the GP image stays installed
    assert all(v == sc.ESTATE for c, v in T["after_set_problem"].items() if c not in ("cesx_gp_predict", "cesx_gp_predict_grad"))
    # the decided cells are written into the header
    text = " ".join(_header().split())
    para = text[text.index("Call order across the families"):]
    para = para[:para.index("*/")]
    for key, (decision, words) in sc.UNDECIDED.items():                      # each decision stands in the header's paragraph, in words
        assert words in para, key
    R = T["lineal_set_behind_a_proposal"]                                    # the re-install behind another family's start: the start stands ...
    assert R["cesx_mh_langevin_propose"] == sc.OK and R["cesx_mh_hmc_begin"] == sc.OK and R["cesx_mh_langevin_run_map"] == sc.OK
    assert R["cesx_mh_langevin_accept"] == sc.ESTATE                         # ... and the pending proposal is over
    assert T["gp_start"]["cesx_mh_run_map"] == sc.OK and T["mh_start"]["cesx_gp_run"] == sc.OK
    assert T["lineal_reinstalled"]["cesx_mh_accept"] == sc.EINVAL
    assert T["gp_langevin_start"]["cesx_mh_langevin_propose"] == sc.OK and T["proj_start"]["cesx_mh_langevin_run_map"] == sc.OK
    assert T["lineal_reinstalled"]["cesx_mh_langevin_lineal_propose"] == sc.ESTATE
    assert T["lineal_reinstalled"]["cesx_mh_langevin_lineal_start"] == sc.OK and T["proposed"]["cesx_gp_langevin_start"] == sc.OK


def test_comparator_sees_one_ulp_and_a_missing_key():
    a = dict(U=np.arange(6.0).reshape(2, 3), cnt=np.arange(3, dtype=np.uint64))
    b = {k: v.copy() for k, v in a.items()}
    assert sc.differences(a, b) == []
    b["U"][1, 2] = np.nextafter(b["U"][1, 2], np.inf)
    assert sc.differences(a, b) == ["U"]
    b["U"][1, 2] = a["U"][1, 2]
    b["U"][0, 0] = -0.0                                                        # bytes, not values
    assert sc.differences(a, b) == ["U"]
    del b["cnt"]
    assert sc.differences(a, b) == ["U", "cnt"]
    assert sc.differences(dict(x=np.zeros(2, np.float32)), dict(x=np.zeros(2, np.float64))) == ["x"]


def test_references_are_the_projects_own():
    """The numpy chains behind the blocks come from the features' case modules; the kinds without one at these shapes are the
    random walks on a forward model, the dense and the projected Sigma."""
    none = {k for k in sc.kinds_of("A") if not any(sc.has_reference("A", k, nz, dt) for nz in sc.NOISES for dt in sc.DTYPES)}
    assert none == {"rw", "pcn", "rw_fused", "gp_dense", "gp_proj", "gp_proj_lv", "gp_proj_hmc"}
    src = open(os.path.join(ROOT, "tests", "sampler_reuse_cases.py")).read()
    for name in ("mlc.np_chains_mala", "hc.np_chains_hmc", "hc.np_chains_hmc_gp", "glc.np_chains_langevin", "llc.np_chains_mala_lineal",
                 "lhc.np_chains", "ac.np_adapt", "gcc.np_chains"):
        assert re.search(re.escape(name) + r"\(", src), name
    # one reference runs here: the injected draws are the draws its numpy chain makes under the block's seed
    sp = sc.spec("A", "map_lv", 1)
    U, acc, _ = sc.reference(sp)
    assert U.shape == sp["U0"].shape and 0 < acc.sum() < sc.n_steps("map_lv") * sp["J"]
    xi, lu = sc.injected(sp)
    np.random.seed(sp["noise_seed"])
    assert np.array_equal(np.random.normal(0, 1, [2, 130]), xi[0]) and np.array_equal(np.log(np.random.uniform(size=130)), lu[0])


def test_stats_plans_vary_and_are_legal():
    for E, e in sc.ENGINES.items():
        plans = [sc.stats_plan(E, i) for i in range(12)]
        assert len({(q["N"], q["bins"], q["lags"], q["chains"], len(q["pairs"])) for q in plans}) >= 8
        assert any(q["abandoned"] for q in plans) and not all(q["abandoned"] for q in plans)
        for q in plans:
            assert q["N"] >= max(4, q["lags"] + 2) and sum(c for c in q["chunks"] if c > 0) == q["N"] and 1 <= q["chains"] <= e["J"]
            assert 2 <= q["bins"] <= 256 and 2 <= q["bins2"] <= 64 and all(a != b and 0 <= a < e["p"] and 0 <= b < e["p"] for a, b in q["pairs"])
