"""The K2 plans, pinned: plan_dense decides which dense kernels a step runs, on which route and how the side stream is joined,
so a change of K2's host code that means to leave the step alone has to leave every plan alone.  Host only (no device)."""
import ctypes
import hashlib
import json
import os

import pytest

from conftest import GOLDEN

NF, NP = 23, 13
(UPDATE, TIME_STEP, PHASE, UPD_OK, F64, P_SLIM, DIAG_SIGMA, CHAIN, HKFREE_OK, UPDATE_V2, HAS_WQ, INFLIGHT, FUSED_CENTER, IMG, SIGNALS,
 IMAGE_ONLY, POLL_JOIN_OK, SHARDED, ON_SIDE, BELOW_SIDE, FUSE_OK, FUSE_AUTO, GRAM_B_SHORT) = range(NF)
# the 16 valid (update, phase, time step) combinations: eks / aldi as a step, aldi_constant as drift and as noise
COMBOS = [(0, 0), (1, 0), (2, 1), (2, 2)]
TIME_STEPS = [0, 1, 2, 4]
# the ten booleans the routes branch on directly (bit i of the case number), and the single switches with the five they meet
FACTORIAL = [INFLIGHT, FUSED_CENTER, IMG, SIGNALS, IMAGE_ONLY, POLL_JOIN_OK, SHARDED, ON_SIDE, BELOW_SIDE, UPD_OK]
SWITCHES = [HKFREE_OK, UPDATE_V2, HAS_WQ, FUSE_OK, FUSE_AUTO, GRAM_B_SHORT]
SWITCH_OVER = [INFLIGHT, FUSED_CENTER, IMG, IMAGE_ONLY, UPD_OK]
UPD = ["eks", "aldi", "aldi_constant"]
TS = ["default", "spectral", "constant", "adaptive", "mix"]
PH = ["step", "drift", "noise"]
ROUTE = ["NoiseOnly", "Tail", "Finish", "General"]
TAIL = ["-", "DenseSigma", "Chained", "Plain"]
JOIN = ["None", "Event", "Polled"]
UPART = ["Side", "Center", "FusedLoad"]
FACTOR = ["None", "Image", "Fp64"]
MODE = ["Aldi", "Eks", "ConstDrift", "ConstNoise"]


@pytest.fixture(scope="module")
def plan():
    from ces_amd import build, engine
    build.build_lib()
    lib = engine.load_library()
    facts, out = (ctypes.c_int32 * NF)(), (ctypes.c_int32 * NP)()

    def plan(f):
        facts[:] = f
        assert lib.cesx_debug_dense_plan(facts, out) == 0, f
        return list(out)
    return plan


@pytest.fixture(scope="module")
def gold():
    with open(os.path.join(GOLDEN, "dense_plan.json")) as fh:
        return json.load(fh)


def base():
    """everything allowed, nothing in flight, no switch given"""
    f = [0] * NF
    for i in (P_SLIM, DIAG_SIGMA, CHAIN, HKFREE_OK, UPDATE_V2, HAS_WQ, SIGNALS, POLL_JOIN_OK, BELOW_SIDE, FUSE_AUTO):
        f[i] = 1
    return f


def group(g):
    f = base()
    f[UPDATE], f[PHASE] = COMBOS[g >> 6]
    f[TIME_STEP] = TIME_STEPS[(g >> 4) & 3]
    f[F64], f[DIAG_SIGMA], f[CHAIN], f[P_SLIM] = (g >> 3) & 1, (g >> 2) & 1, (g >> 1) & 1, g & 1
    return f


def group_name(g):
    f = group(g)
    return "%s/%s/%s f64 %d diag_sigma %d chain %d slim %d" % (UPD[f[UPDATE]], PH[f[PHASE]], TS[f[TIME_STEP]], f[F64], f[DIAG_SIGMA],
                                                                f[CHAIN], f[P_SLIM])


def digest(plan, f, over, h=None):
    h = h or hashlib.sha256()
    for k in range(1 << len(over)):
        for b, i in enumerate(over):
            f[i] = (k >> b) & 1
        h.update(("".join("%d " % v for v in f) + ":" + "".join(" %d" % v for v in plan(f)) + "\n").encode())
    return h


def test_dense_plans_are_the_recorded_ones(plan, gold):
    """cesx_debug_dense_plan gives, for every case of the sweep -- the 16 valid (update, phase, time step) combinations x 2 dtypes
    x diag_sigma x chain x both sides of potrf_ld(p) <= 256, each with the full factorial over the ten booleans the routes
    branch on (unreachable combinations included: the function is pure) --, the plan recorded in tests/golden/dense_plan.json:
    one digest per group of 1024 (tools/make_golden_dense_plans.py; written from the commit BEFORE plan_dense existed, from its
    launch_dense conditions, and never regenerated from a tree that changes them)."""
    assert len(gold["groups"]) == 256 and gold["cases"] == 256 * 1024 + 6 * 256 * 32
    bad = []
    for g in range(256):
        h = digest(plan, group(g), FACTORIAL)
        if h.hexdigest()[:16] != gold["groups"][g]:
            bad.append(group_name(g))
    assert not bad, bad


def test_dense_plans_with_one_switch_off_are_the_recorded_ones(plan, gold):
    """The same with one input away from its base value -- hk-free not allowed, no LDS-DMA update kernels, no image allocated,
    CESX_FUSE_CENTER=1, CESX_FUSE_CENTER=0, a short second Gram launch --: every group x the 32 settings of {in flight, centring
    fused, L into the image, d_L left out, an update kernel takes the image}; one digest per switch."""
    assert len(gold["switches"]) == len(SWITCHES)
    for k, sw in enumerate(SWITCHES):
        h = hashlib.sha256()
        for g in range(256):
            f = group(g)
            f[sw] ^= 1
            digest(plan, f, SWITCH_OVER, h)
        assert h.hexdigest()[:16] == gold["switches"][k], "switch %d (fact %d)" % (k, sw)


def test_dense_plans_of_the_benchmark_state_by_name(plan, gold):
    """The 16 plans of the benchmark's engine in its steady state (fp32, p = 256, diagonal Sigma, chained image; chol(C) in flight
    with its own centring launch, L into the image for aldi, d_L left out behind a tail step), readable in the fixture."""
    got = []
    for upd, ph in COMBOS:
        for ts in TIME_STEPS:
            f = base()
            f[UPDATE], f[PHASE], f[TIME_STEP], f[UPD_OK] = upd, ph, ts, 1
            f[INFLIGHT] = int(ph != 2)
            f[IMG] = int(upd == 1)
            f[IMAGE_ONLY] = int(f[IMG] and ts == 0)
            p = plan(f)
            got.append("%s/%s/%s: route %s tail %s join %s upart %s center %d factor %s refactor %d gemm_M %d spectral %d "
                       "gain_inverse %d eks_inverse %d mode %s ktot %d"
                       % (UPD[upd], PH[ph], TS[ts], ROUTE[p[0]], TAIL[p[1]], JOIN[p[2]], UPART[p[3]], p[4], FACTOR[p[5]], p[6], p[7],
                          p[8], p[9], p[10], MODE[p[11]], p[12]))
    assert got == gold["bench"]
    # the benchmark's own step: the chained tail launch polls for the side stream, nothing else runs on the caller's stream
    assert gold["bench"][4].startswith("aldi/step/default: route Tail tail Chained join Polled upart Side center 0 factor None")


def test_dense_plan_rejects_bad_facts(plan):
    from ces_amd import engine
    lib = engine.load_library()
    out = (ctypes.c_int32 * NP)()
    for i, v in ((UPDATE, 3), (TIME_STEP, 5), (PHASE, 3), (UPDATE, -1)):
        f = base()
        f[i] = v
        assert lib.cesx_debug_dense_plan((ctypes.c_int32 * NF)(*f), out) < 0
    assert lib.cesx_debug_dense_plan(None, out) < 0
