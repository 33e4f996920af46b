"""The Calibrate stage -- K1 Gram (kernels_gram*.hip), K2 dense algebra (kernels_dense.hip), K3 update (kernels_update*.hip) --
term by term against fp64 at its ragged, strided and picker edges.

Every kernel stage is compared with the staged reference of oracle/calibrate_ref.py computed FROM WHAT THAT STAGE READ: the
inputs rounded to the engine dtype on the host and the device's own output of the stage before (the moment buffer for K2;
cesx_debug_dense and hk for K3; the drift of aldi_constant's first pass for its second).  The bar is ELEMENTWISE,

    |dev - ref| <= c * eps * B     for every entry,

eps the unit roundoff of the engine dtype, B the reference's expression in absolute values, c the derived worst-case constant
of the sums the kernel forms (c_update = ktot + 8, c_gram = the particles of one slab + 4, c_metric: derivations in oracle/calibrate_ref.py).  K2 is
fp64 on both engine dtypes and is held to BAND = 1e-9 relative to each array's maximum.  Nothing here was fitted to a device:
tests/test_calibrate_refs_host.py shows on these very case tables that numpy in the engine dtype stays inside the bound and
that every mutant of calibrate_ref.mutants leaves 4x the bound in at least one of the two problem families -- every K3
case runs in BOTH ('data': today's synthetic problem, data and noise carry the step; 'prior': the prior, mu and alpha terms
carry it).

Which kernel ran: cesx_debug_update_form tells the three ALDI forms apart and is asserted.  update2_kernel / update2s_kernel
/ update3_kernel / update3s_kernel / update_kernel and the Gram arms (gram2_kernel sg / imm, the v1 Gram) cannot be told
apart from outside; ``pick`` below restates pick_update_kernel, update4_shape_ok, plan_dense's tail route and update2_lds /
update3_lds, the case tables carry the kernel the restatement names, and the shapes sit on both sides of every border so that
the picker's source leaves no doubt; the Gram arm of a launch follows from its PLAN (``k1_launches``).  The measured worst
ratios |err| / (eps B) are printed per part when the module ends (NOTEBOOK.md, "Calibrate: edges"); a record, not the bar."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from edge_helpers import guarded, guards_intact, put  # noqa: E402

from oracle import calibrate_ref as cr  # noqa: E402

gpu = pytest.mark.gpu            # every test that launches a kernel; the case-table test below needs no device

SEED = 77
STEP = 5                         # Philox step index of the noise block the engine draws
WORST = {}                       # part -> [derived c, worst |err| / (eps B), cases]


@pytest.fixture(scope="module")
def eng_mod():
    """The engine module; when the module's tests are over, the worst ratios of THIS run go on record (per kernel and family:
    the derived c, the worst measured |err| / (eps B); K2: worst error / BAND) -- whatever subset was selected."""
    import torch
    from ces_amd import engine
    assert torch.cuda.is_available(), "these tests need the MI355X"
    yield engine
    for part in sorted(WORST):
        c, ratio, cases = WORST[part]
        print("\nCALIBRATE-EDGES %-44s c = %6d   worst |err| / (eps B) = %10.4g   (%d comparisons)" % (part, c, ratio, cases), end="")
    print()


def gram_plan(p, n, J, dtype):
    """plan(part, budget) -> info of cesx_debug_gram_plan (host only: needs the library, not a device)."""
    import ctypes
    from ces_amd import engine
    lib = engine.load_library()

    def plan(part, budget):
        info = (ctypes.c_int * 6)()
        assert lib.cesx_debug_gram_plan(p, n, 0 if dtype == "float32" else 1, part, budget, J, info) == 0
        return list(info)
    return plan


def k1_launches(c, cus=256):
    """Per Gram launch of a K1 case: (staged rows, kernel arm, replanned) -- pick_gram_kernel restated: gram2_kernel when J is
    whole tiles and U, G are 16-byte aligned, its imm arm up to 480 staged rows (max_rb * tile of the PLAN, not p + n), the
    other arm up to 512; otherwise the v1 Gram.  replanned: plan_gram_parts plans that launch again (oracle/calibrate_ref.py)."""
    tile = kt = 32 if c["dtype"] == "float32" else 16
    out = []
    for info, replanned in cr.gram_plans(c["p"], c["n"], c["J"], c["dtype"], cus, gram_plan(c["p"], c["n"], c["J"], c["dtype"])):
        if info[0] == 0:
            continue
        rows = info[4] * tile
        g2 = c["J"] % kt == 0 and c["J"] >= kt and c["shift"] == 0 and rows <= 512
        out.append((rows, ("gram2_imm" if rows <= 480 else "gram2") if g2 else "v1", replanned))
    return out


# ---- the pickers, restated (kernels_update.hip pick_update_kernel, kernels_update4.hip update4_shape_ok,
#      kernels_dense.hip plan_dense / image_ok, kernels_update2.hip update2_lds, kernels_update3.hip update3_lds) ----------

U2_LDS_MAX, U3_LDS_MAX = 80 * 1024, 78 * 1024


def update2_lds(kn):
    return 3 * (16 * 1024 + 8 * 1024) + kn * 16          # U2_RING (U2_WSLOT + U2_XSLOT) + kn 16


def update3_lds(kn):
    return 3 * 8 * 1024 + 256 * 64 + kn * 32              # U3_RING U3_XSLOT + U3_THREADS 64 + kn 32


def pick(p, n, J, dtype, update="aldi", time_step=None, dense_sigma=False, aligned=True, noise_in_kernel=False):
    """(update form, kernel) of the main launch of a step (aldi_constant: of its drift launch, [U | G])."""
    f32 = np.dtype(dtype) == np.float32
    kp, kn = cr.pad16(p), cr.pad16(n)
    rpad = (max(p, n) + 255) // 256 * 256
    drift = update == "aldi_constant"
    lds_ok = update2_lds(kn) <= U2_LDS_MAX if f32 else (not (noise_in_kernel and not drift) and update3_lds(kn) <= U3_LDS_MAX)
    dma = J % 4 == 0 and J >= 4 and aligned and lds_ok
    image_ok = f32 and update == "aldi" and time_step is None and (p + 31) // 32 * 32 <= 256       # image_ok: potrf_ld(p) <= 256
    chain = image_ok and not dense_sigma and 224 < p <= 256 and rpad == 256 and kn <= 256 and J % 4 == 0 and 4 <= J < (1 << 26)
    form = 1 if image_ok and dma else 0
    if form == 1 and chain:
        return 2, "update4"
    if not dma:
        return form, "update_aligned" if (J % (4 if f32 else 2) == 0 and aligned) else "update_unaligned"
    small = p <= 64 and ((kp + kn) if drift else (2 * kp + kn)) // 16 <= 12       # out_rows <= 64, U2S_MAX_KT / U3S_MAX_KT
    return form, ("update2" if f32 else "update3") + ("s" if small else "")


def jmin(p):
    """the smallest multiple of 4 above p + 1 (C = cov(U) + 1e-8 I needs J - 1 >= p to be well defined)"""
    return 4 * ((p + 1) // 4 + 1)


# ---- K3 case tables -------------------------------------------------------------------------------------------------------

def k3(p, n, J, dtype="float32", update="aldi", ts=None, xi="injected", dg=False, ds=False, shift=0, kernel=None, form=None):
    """One K3 case.  xi: 'injected' | 'ahead' (cesx_step draws it on the side stream) | 'engine' (cesx_apply finds no block and
    draws it itself); dg / ds: dense Gamma / Sigma; shift: U, G, xi and the output start that many elements off 16-byte
    alignment, inside sentinel guards (0: plain tensors)."""
    c = dict(p=p, n=n, J=J, dtype=dtype, update=update, ts=ts, xi=xi, dg=dg, ds=ds, shift=shift)
    f, k = pick(p, n, J, dtype, update, ts, ds, aligned=shift == 0, noise_in_kernel=(xi == "engine"))
    c["form"], c["kernel"] = (f if form is None else form), (k if kernel is None else kernel)
    return c


U4_P, U4_N = (225, 232, 249, 256), (1, 15, 16, 17, 255, 256)
# update4_kernel: every (p, n) pair once, every J at every p and at all but a few n (a Latin arrangement of the full cross)
K3_UPDATE4 = [k3(p, n, (jmin(p), 288, 1028, 4100)[(i + k) % 4]) for i, p in enumerate(U4_P) for k, n in enumerate(U4_N)]
K3_UPDATE4 += [k3(256, 256, 4096), k3(256, 256, 1028), k3(225, 1, 232), k3(249, 17, 288), k3(232, 255, 4100), k3(256, 15, 260),
               k3(256, 64, 1028, xi="ahead"), k3(233, 37, 288, xi="ahead"), k3(256, 64, 1028, xi="engine"), k3(249, 17, jmin(249), xi="engine")]
K3_UPDATE4 = [c for i, c in enumerate(K3_UPDATE4) if c not in K3_UPDATE4[:i]]          # (the Latin arrangement already holds some of the named shapes)
# just outside update4_kernel: another kernel, the same reference
K3_OUTSIDE4 = [k3(224, 64, 1028), k3(257, 64, 1028), k3(256, 257, 1028), k3(256, 64, 1030), k3(256, 64, 1028, dtype="float64"),
               k3(256, 64, 1028, ts="constant")]
# the LDS-DMA kernels: small | tiled (out_rows 64 | 65, ktot 192 | 208), two row chunks, hk-free against assembled, the LDS border
K3_DMA = []
for _dt in ("float32", "float64"):
    K3_DMA += [k3(64, 64, 512, _dt), k3(64, 65, 512, _dt), k3(65, 64, 512, _dt), k3(16, 150, 516, _dt), k3(16, 161, 516, _dt),
               k3(257, 40, 1028, _dt), k3(300, 40, 1004, _dt), k3(512, 24, 1028, _dt),
               k3(64, 64, 512, _dt, ts="constant"), k3(96, 80, 1028, _dt), k3(96, 80, 1028, _dt, ts="constant"),
               k3(64, 50, 1028, _dt, update="eks"), k3(250, 100, 1028, _dt, update="eks"), k3(33, 17, 132, _dt, update="eks"),
               k3(64, 50, 1028, _dt, update="aldi_constant"), k3(256, 64, 1028, _dt, update="aldi_constant"),
               k3(33, 17, 132, _dt, xi="ahead"), k3(64, 64, 512, _dt, xi="engine")]
K3_DMA += [k3(8, 512, 260), k3(8, 513, 260), k3(8, 1216, 260, "float64"), k3(8, 1217, 260, "float64")]
# update_kernel, the fallback: J = 4k + 1, 2, 3, both template arms, unaligned views inside guards
K3_GENERIC = []
for _dt in ("float32", "float64"):
    K3_GENERIC += [k3(33, 17, 129, _dt), k3(33, 17, 130, _dt), k3(33, 17, 131, _dt), k3(300, 40, 1001, _dt),
                   k3(33, 17, 132, _dt, shift=1), k3(33, 17, 132, _dt, shift=3), k3(64, 50, 1028, _dt, shift=1),
                   k3(33, 17, 131, _dt, update="aldi_constant"), k3(33, 17, 130, _dt, update="eks"),
                   k3(250, 100, 1028, _dt, shift=3)]
# dense Gamma: the whitening launch (out_rows = n, a triangular segment) in front; dense Sigma: M = C Sigma^{-1} rows in the tail
K3_DENSE = []
for _dt in ("float32", "float64"):
    K3_DENSE += [k3(40, n, 1028, _dt, dg=True) for n in (17, 64, 65, 256)]
    K3_DENSE += [k3(p, 40, 1028, _dt, ds=True) for p in (33, 250, 256)]
    K3_DENSE += [k3(40, 65, 1028, _dt, update="eks", dg=True, ds=True), k3(40, 64, 1030, _dt, dg=True)]
K3_CASES = K3_UPDATE4 + K3_OUTSIDE4 + K3_DMA + K3_GENERIC + K3_DENSE


def k3_id(c):
    s = "%s-p%d-n%d-J%d-%s" % (c["dtype"][-2:], c["p"], c["n"], c["J"], c["update"])
    for key, tag in (("ts", "ts_%s"), ("dg", "denseGamma"), ("ds", "denseSigma"), ("shift", "off%s")):
        if c[key]:
            s += "-" + (tag % c[key] if "%" in tag else tag)
    return s + ("" if c["xi"] == "injected" else "-xi_" + c["xi"]) + "-" + c["kernel"]


# ---- K1 / K2 case tables --------------------------------------------------------------------------------------------------

def k1(p, n, J, dtype="float32", shift=0, far=False):
    kt = 32 if dtype == "float32" else 16
    return dict(p=p, n=n, J=J, dtype=dtype, shift=shift, far=far, tiles=J % kt == 0 and J >= kt and shift == 0,
                sg=p % 8 == 0 and (p + n) % 8 == 0)


K1_CASES = [k1(64, 64, 32), k1(64, 64, 33), k1(64, 64, 64), k1(64, 64, 4096), k1(64, 64, 4100), k1(64, 50, 1024), k1(60, 68, 1024),
            k1(33, 17, 1024), k1(33, 17, 131), k1(64, 64, 1024, shift=1), k1(64, 50, 1028, shift=3),
            k1(256, 224, 1024), k1(256, 225, 1024), k1(256, 256, 1024), k1(256, 257, 1024), k1(300, 260, 1024), k1(225, 1, 1028),
            k1(480, 32, 1024), k1(448, 64, 1024),
            k1(64, 64, 1024, far=True), k1(33, 17, 131, far=True),
            k1(64, 64, 16, "float64"), k1(64, 64, 17, "float64"), k1(64, 64, 1024, "float64"), k1(64, 64, 1032, "float64"),
            k1(64, 50, 1024, "float64"), k1(48, 17, 1024, "float64"), k1(33, 17, 131, "float64"), k1(64, 64, 1024, "float64", shift=1),
            k1(256, 224, 512, "float64"), k1(256, 225, 512, "float64"), k1(256, 256, 512, "float64"), k1(256, 257, 512, "float64"),
            k1(480, 32, 512, "float64"), k1(496, 16, 512, "float64"),
            k1(64, 64, 1024, "float64", far=True)]


def k1_id(c):
    return "%s-p%d-n%d-J%d%s%s" % (c["dtype"][-2:], c["p"], c["n"], c["J"], "-off%d" % c["shift"] if c["shift"] else "", "-far" if c["far"] else "")


TS_RULES = {
    "default": (dict(time_step=None), []),
    "spectral": (dict(time_step="spectral"), []),
    "constant_dt": (dict(time_step="constant", delta_t=0.02), [0.4]),
    "constant_default": (dict(time_step="constant"), []),
    "mix_spinup_done": (dict(time_step="mix", delta_t=0.05, spinup=0.5), [0.3, 0.9]),
    "mix_late_recompute": (dict(time_step="mix", delta_t=0.05, spinup=2.0), [1.2, 2.5]),
    "mix_before_spinup": (dict(time_step="mix", delta_t=0.05, spinup=4.0), [0.2]),
}
POTRF_P = (1, 7, 8, 9, 16, 17, 255, 256, 257, 260, 512)          # potrf_reg_kernel up to 256 (potrf_ld 32 .. 256), blocked above


def k2(p, n, J, dtype, update="aldi", rule="default", dg=False, ds=False, fam="prior"):
    return dict(p=p, n=n, J=J, dtype=dtype, update=update, rule=rule, dg=dg, ds=ds, fam=fam)


K2_CASES = [k2(p, 24, 4 * ((2 * p + 72) // 4), dt, fam=("prior", "data")[i % 2]) for i, p in enumerate(POTRF_P) for dt in ("float32", "float64")]
K2_CASES += [k2(64, 50, 1028, dt, upd, rule, fam=fam) for dt in ("float32", "float64") for upd in ("aldi", "eks") for rule in sorted(TS_RULES)
             for fam in ("prior",)]
K2_CASES += [k2(256, 64, 1028, "float32", upd, rule, fam="data") for upd in ("aldi", "eks") for rule in sorted(TS_RULES)]
K2_CASES += [k2(48, 40, 1028, dt, upd, rule, dg=True, ds=True) for dt in ("float32", "float64") for upd in ("aldi", "eks")
             for rule in ("default", "spectral", "constant_dt", "mix_late_recompute")]
K2_CASES += [k2(64, 50, 1028, dt, "aldi_constant", dg=dg, ds=ds) for dt in ("float32", "float64") for dg, ds in ((False, False), (True, False), (False, True))]
K2_CASES += [k2(300, 40, 1028, "float64", "eks", "constant_dt", ds=True), k2(257, 17, 1028, "float32", "aldi", "default", dg=True)]


def k2_id(c):
    return "%s-p%d-n%d-J%d-%s-%s-%s%s%s" % (c["dtype"][-2:], c["p"], c["n"], c["J"], c["update"], c["rule"], c["fam"],
                                            "-denseGamma" if c["dg"] else "", "-denseSigma" if c["ds"] else "")


# ---- the case tables hold every border they were built for ------------------------------------------------------------------

def test_the_case_tables_cover_what_they_must():
    """Host-side (needs no device): a later edit cannot thin the tables out silently."""
    def has(cases, **kw):
        return any(all(c[k] == v for k, v in kw.items()) for c in cases)
    # the LDS borders, derived from the *_lds functions: fp32 padded n 512 | 528, fp64 1216 | 1232
    assert update2_lds(512) <= U2_LDS_MAX < update2_lds(528) and update3_lds(1216) <= U3_LDS_MAX < update3_lds(1232)
    assert pick(8, 512, 260, "float32")[1] == "update2" and pick(8, 513, 260, "float32")[1] == "update_aligned"
    assert pick(8, 1216, 260, "float64")[1] == "update3" and pick(8, 1217, 260, "float64")[1] == "update_aligned"
    for n in (512, 513):
        assert has(K3_DMA, n=n, dtype="float32")
    for n in (1216, 1217):
        assert has(K3_DMA, n=n, dtype="float64")
    # update4_kernel: every p (partial last 32-row block, partial last 8-column panel), n and J border; all three noise sources
    u4 = [c for c in K3_UPDATE4]
    assert all(c["kernel"] == "update4" and c["form"] == 2 and c["dtype"] == "float32" for c in u4)
    for p in U4_P:
        for n in U4_N:
            assert has(u4, p=p, n=n)
        for J in (jmin(p), 288, 1028, 4100):
            assert has(u4, p=p, J=J), (p, J)
    assert [jmin(p) for p in U4_P] == [228, 236, 252, 260]
    assert all(jmin(p) < 128 + jmin(p) % 128 + 256 for p in U4_P)          # fewer particles than three workgroups of 128 take
    for xi in ("injected", "ahead", "engine"):
        assert has(u4, xi=xi)
    # just outside: p = 224, p = 257, n = 257, J % 4 = 2, fp64, another time step -- none of them the chained form
    out = {(c["p"], c["n"], c["J"], c["dtype"], c["ts"]): (c["form"], c["kernel"]) for c in K3_OUTSIDE4}
    assert out[(224, 64, 1028, "float32", None)] == (1, "update2") and out[(257, 64, 1028, "float32", None)] == (0, "update2")
    assert out[(256, 257, 1028, "float32", None)] == (1, "update2") and out[(256, 64, 1030, "float32", None)] == (0, "update_unaligned")
    assert out[(256, 64, 1028, "float64", None)] == (0, "update3") and out[(256, 64, 1028, "float32", "constant")] == (0, "update2")
    # small | tiled: out_rows 64 | 65, ktot 192 | 208; two row chunks; hk-free against assembled; eks; aldi_constant
    for dt, stem in (("float32", "update2"), ("float64", "update3")):
        kern = {(c["p"], c["n"], c["update"], c["ts"]): c["kernel"] for c in K3_DMA if c["dtype"] == dt and c["xi"] == "injected"}
        assert kern[(64, 64, "aldi", None)] == stem + "s" and kern[(64, 65, "aldi", None)] == stem and kern[(65, 64, "aldi", None)] == stem
        assert kern[(16, 150, "aldi", None)] == stem + "s" and kern[(16, 161, "aldi", None)] == stem
        assert cr.ktot(64, 64) == 192 and cr.ktot(64, 65) == 208 and cr.ktot(16, 150) == 192 and cr.ktot(16, 161) == 208
        for p in (257, 300, 512):
            assert kern[(p, 40 if p != 512 else 24, "aldi", None)] == stem
        for upd in ("eks", "aldi_constant"):
            assert has(K3_DMA, dtype=dt, update=upd)
        forms = {(c["p"], c["ts"]): c["form"] for c in K3_DMA if c["dtype"] == dt and c["update"] == "aldi" and c["xi"] == "injected"}
        assert forms[(96, None)] == (1 if dt == "float32" else 0) and forms[(96, "constant")] == 0
    # the fallback: J = 4k + 1, 2, 3, both template arms, unaligned views
    for dt in ("float32", "float64"):
        g = [c for c in K3_GENERIC if c["dtype"] == dt]
        assert {c["J"] % 4 for c in g} >= {1, 2, 3} and {c["shift"] for c in g} >= {1, 3}
        assert all(c["kernel"].startswith("update_") and c["form"] == 0 for c in g)
    assert has(K3_GENERIC, kernel="update_aligned") and has(K3_GENERIC, kernel="update_unaligned")
    assert has(K3_DMA, kernel="update_aligned", dtype="float32") and has(K3_DMA, kernel="update_aligned", dtype="float64")
    # dense Gamma at n = 17, 64, 65, 256; dense Sigma at p = 33, 250, 256, where 256 must not take the chained form
    for dt in ("float32", "float64"):
        for n in (17, 64, 65, 256):
            assert has(K3_DENSE, dtype=dt, dg=True, n=n)
        for p in (33, 250, 256):
            assert has(K3_DENSE, dtype=dt, ds=True, p=p)
    assert all(c["form"] == 1 for c in K3_DENSE if c["dtype"] == "float32" and c["ds"] and c["update"] == "aldi")
    ids = [k3_id(c) for c in K3_CASES]
    assert len(set(ids)) == len(ids)
    # K1: J % 32 (fp32) / J % 16 (fp64) zero and not, one tile and one tile + 1, unaligned views, the sg arm's % 8, a last
    # 32-row block of one row, a shift far from the mean; staged rows up to 480 (the imm arm) and 481 .. 512 (the other), read
    # from the PLAN of launches cesx_create does not plan again; p + n above 512 (rectangles: gram2 still runs)
    for dt, kt in (("float32", 32), ("float64", 16)):
        k = [c for c in K1_CASES if c["dtype"] == dt]
        assert has(k, J=kt, tiles=True) and has(k, J=kt + 1, tiles=False) and has(k, shift=1, tiles=False) and has(k, far=True)
        assert any(c["J"] % kt == 0 and c["J"] > kt for c in k) and any(c["J"] % kt != 0 and c["J"] > 1024 for c in k)
        assert has(k, sg=True, tiles=True) and has(k, sg=False, tiles=True)
        arms = [(rows, arm) for c in k for rows, arm, replanned in k1_launches(c) if not replanned]
        assert any(arm == "gram2_imm" and rows == 480 for rows, arm in arms) and any(arm == "gram2_imm" and rows < 480 for rows, arm in arms)
        assert any(arm == "gram2" and 480 < rows <= 512 for rows, arm in arms) and any(arm == "v1" for rows, arm in arms)
        assert all(rows <= 512 for rows, arm in arms)
        assert any(c["p"] + c["n"] > 512 and all(arm != "v1" for _, arm, _ in k1_launches(c)) for c in k)
        # the chain the bound is built from: one tile per slab where the plan pins it (always at the large J, where a chain of
        # all of J could not see one lost particle), all of J where the launch is re-planned or the slices cannot be pinned
        for c in k:
            chain = cr.gram_chain(c["p"], c["n"], c["J"], dt, 256, gram_plan(c["p"], c["n"], c["J"], dt))
            assert min(kt, c["J"]) <= chain <= c["J"] and (c["J"] <= 1100 or chain == kt), (k1_id(c), chain)
    assert has(K1_CASES, p=60, n=68, sg=False) and has(K1_CASES, p=64, n=50, sg=False)       # p % 8 and (p + n) % 8, each alone
    assert (256 + 225) % 32 == 1 and (48 + 17) % 16 == 1 and has(K1_CASES, p=48, n=17, dtype="float64")
    assert len({k1_id(c) for c in K1_CASES}) == len(K1_CASES)
    # K2: every factorisation size on both routes, every time-step rule, dense Gamma and dense Sigma
    for dt in ("float32", "float64"):
        assert {c["p"] for c in K2_CASES if c["dtype"] == dt and c["rule"] == "default" and c["update"] == "aldi"} >= set(POTRF_P)
        for upd in ("aldi", "eks"):
            assert {c["rule"] for c in K2_CASES if c["dtype"] == dt and c["update"] == upd} == set(TS_RULES)
        assert has(K2_CASES, dtype=dt, dg=True, ds=True) and has(K2_CASES, dtype=dt, update="aldi_constant")
    assert len({k2_id(c) for c in K2_CASES}) == len(K2_CASES)


# ---- running a case ---------------------------------------------------------------------------------------------------------

def note(part, c, ratio):
    w = WORST.setdefault(part, [c, 0.0, 0])
    w[0], w[1], w[2] = max(w[0], c), max(w[1], ratio), w[2] + 1


def held(dev, ref, B, c, eps, label, part, extra=0.0):
    """|dev - ref| <= (c eps + extra) B for every entry; the worst |err| / (eps B) goes on record."""
    dev, ref, B = (np.asarray(a, dtype=np.float64) for a in (dev, ref, B))
    assert dev.shape == ref.shape == B.shape and np.all(np.isfinite(dev)), (label, "shape or a non-finite value")
    err = np.abs(dev - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(B > 0, err / (eps * B), np.where(err > 0, np.inf, 0.0))
    worst = float(ratio.max()) if ratio.size else 0.0
    note(part, c, worst)
    print("%s [%s]: worst |err| / (eps B) = %.3g, c = %d" % (label, part, worst, c))
    bad = err > (c * eps + extra) * B
    assert not bad.any(), (label, part, "entries over the bound: %d, first %s, worst ratio %.4g against c = %d"
                           % (int(bad.sum()), tuple(np.argwhere(bad)[0]), worst, c))


def buffers(eng, d, shift):
    """U, G, xi and the output on the device: plain tensors, or views ``shift`` elements into guarded buffers."""
    import torch
    if not shift:
        mk = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=eng.np_dtype), device=eng.device)      # noqa: E731
        return None, mk(d["U0"]), mk(d["G"]), mk(d["xi"]), eng.empty(eng.p)
    flats, views = [], []
    for rows, key in ((eng.p, "U0"), (eng.n_obs, "G"), (eng.p, "xi"), (eng.p, None)):
        f, v = guarded(eng, rows, shift)
        if key:
            put(v, d[key].astype(eng.np_dtype))
        flats.append(f)
        views.append(v)
    return list(zip(flats, views)), views[0], views[1], views[2], views[3]


def problem_of(c, fam):
    return cr.family(fam, c["p"], c["n"], c["J"], c["dtype"], dense_gamma=c["dg"], dense_sigma=c["ds"])


def run_k3(eng_mod, c, fam):
    import torch
    p, n, J, dtype = c["p"], c["n"], c["J"], c["dtype"]
    eps, label = cr.eps_of(dtype), k3_id(c) + "/" + fam
    d = problem_of(c, fam)
    eng = eng_mod.Engine(p, n, J, dtype=dtype, seed=SEED)
    eng.set_problem(d["y"], d["Gamma"], d["mu"], d["sigma"], d["ustar"])
    guards, U, G, xi_t, out = buffers(eng, d, c["shift"])
    prm = eng_mod.step_params(update=c["update"], time_step=c["ts"], step_index=STEP)
    cu = cr.c_update(p, n, dense_gamma=c["dg"])
    if c["xi"] == "injected":
        xi_h = d["xi"]
    else:
        xi_t, xi_h = None, eng.draw_noise(STEP).cpu().numpy().astype(np.float64)
    part = c["kernel"] + "/" + fam
    if c["update"] == "aldi_constant":
        # both passes through the split entry points, so that the drift and its maximum can be read between them
        eng.set_shift(eng.colsum(U, G))
        mom = eng.moments(U, G)
        absmax = eng.apply_drift(prm, mom, U, G, out)
        torch.cuda.synchronize()
        drift = out.cpu().numpy().astype(np.float64)
        dd = eng.debug_dense()
        ref, B = cr.update_ref("drift", dd, None, d["U0"], d["G"], None, d, J=J)
        held(drift, ref, B, cu, eps, label + " drift", part)
        assert float(absmax.cpu()[0]) == np.max(np.abs(drift)), (label, "max|drift|")
        if c["xi"] == "ahead":
            eng.prefetch_noise(STEP)
        eng.apply_finish(prm, absmax, U, xi_t, out)
        res = eng.result()
        assert res.hk == pytest.approx(0.1 / np.max(np.abs(drift)), rel=1e-15)
        ref, B = cr.update_ref("finish", dd, res.hk, d["U0"], None, xi_h, d, J=J, drift=drift)
        held(out.cpu().numpy(), ref, B, cu, eps, label + " finish", part)
    else:
        if c["xi"] == "engine":            # no block injected, none drawn ahead: cesx_apply has the update launch draw it
            eng.set_shift(eng.colsum(U, G))
            mom = eng.moments(U, G)
            eng.apply(prm, mom, U, G, None, out=out)
        else:
            eng.step(prm, U, G, xi=xi_t, out=out)
        res = eng.result()
        got_form = eng.update_form()
        assert got_form == c["form"], (label, "update form", got_form)
        dd = eng.debug_dense()
        form = "eks" if c["update"] == "eks" else cr.FORM_OF_UPDATE_FORM[got_form]
        ref, B = cr.update_ref(form, dd, res.hk, d["U0"], d["G"], xi_h, d, J=J)
        # (eks: P = (I + hk M)^{-1} and P K are K2 products without a read-back, held to K2's bar: oracle/calibrate_ref.py)
        held(out.cpu().numpy(), ref, B, cu, eps, label, part, extra=cr.BAND if form == "eks" else 0.0)
    if guards:
        for f, v in guards:
            assert guards_intact(f, v), (label, "written outside a buffer")
        assert np.array_equal(U.cpu().numpy().astype(np.float64), d["U0"]) and np.array_equal(G.cpu().numpy().astype(np.float64), d["G"])
    # the per-particle data metrics K3 sums while the G rows stream by (a dense Gamma: the rows of the whitening launch)
    Lg, Li = cr.whitening(d["Gamma"])
    if Lg is None:
        m = cr.data_metrics_ref(d["G"], dd["gbar"], d["y"], 1.0 / np.diag(d["Gamma"]))
    else:
        m = cr.data_metrics_ref(Li @ d["G"], Li @ dd["gbar"], Li @ d["y"], np.ones(n), G_abs=np.abs(Li) @ np.abs(d["G"]))
    cm = cr.c_metric(n, dense_gamma=c["dg"])
    for key in ("bias_data", "self_bias_data"):
        val, scale = m[key]
        ratio = abs(getattr(res, key) - val) / (eps * scale)
        note("metrics/" + c["kernel"] + ("/denseGamma" if c["dg"] else ""), cm, ratio)
        assert ratio <= cm, (label, key, getattr(res, key), val, ratio, cm)
    eng.close()


@gpu
@pytest.mark.parametrize("fam", cr.FAMILIES)
@pytest.mark.parametrize("c", K3_UPDATE4 + K3_OUTSIDE4, ids=k3_id)
def test_update4_kernel_and_its_neighbours(eng_mod, c, fam):
    """K3 through the Cholesky factor (kernels_update4.hip: fp32, 224 < p <= 256, n <= 256, J % 4 = 0) at its partial last 32-row
    block and 8-column panel, its ragged G tile, fewer particles than a workgroup takes and a last block of 4, with the noise
    injected, drawn ahead and drawn by the engine -- and the shapes just outside, which run another kernel."""
    run_k3(eng_mod, c, fam)


@gpu
@pytest.mark.parametrize("fam", cr.FAMILIES)
@pytest.mark.parametrize("c", K3_DMA, ids=k3_id)
def test_lds_dma_update_kernels_at_their_borders(eng_mod, c, fam):
    """update2_kernel / update2s_kernel (fp32), update3_kernel / update3s_kernel (fp64): small | tiled, two row chunks, the LDS
    border, the hk-free against the assembled image, eks, both passes of aldi_constant with max|drift|."""
    run_k3(eng_mod, c, fam)


@gpu
@pytest.mark.parametrize("fam", cr.FAMILIES)
@pytest.mark.parametrize("c", K3_GENERIC, ids=k3_id)
def test_fallback_update_kernel_ragged_and_unaligned(eng_mod, c, fam):
    """update_kernel: J = 4k + 1, 2, 3, both ``aligned`` arms, and inputs / output 1 and 3 elements off 16-byte alignment inside
    sentinel guards that must be intact afterwards (inputs unchanged as well)."""
    run_k3(eng_mod, c, fam)


@gpu
@pytest.mark.parametrize("fam", cr.FAMILIES)
@pytest.mark.parametrize("c", K3_DENSE, ids=k3_id)
def test_dense_gamma_and_dense_sigma_updates(eng_mod, c, fam):
    """A dense Gamma (the whitening launch in front: out_rows = n, a triangular segment; its rounding is part of the bound) and
    a dense Sigma (M = C Sigma^{-1} formed row by row in the tail launch; p = 256 must not take the chained form)."""
    run_k3(eng_mod, c, fam)


@gpu
@pytest.mark.parametrize("c", K1_CASES, ids=k1_id)
def test_gram_kernels_at_their_edges(eng_mod, c):
    """K1: the packed moment buffer against fp64 sums of the shifted rounded data, entry by entry, with the shift the test set
    itself (cesx_colsum -> cesx_set_shift, restated exactly: set_shift_kernel rounds sums / N to the engine dtype); the row sums
    of cesx_colsum; cesx_moments_uu + cesx_moments_rest bit-identical to cesx_moments; guards around unaligned views intact."""
    import torch
    p, n, J, dtype = c["p"], c["n"], c["J"], c["dtype"]
    eps, label = cr.eps_of(dtype), k1_id(c)
    d = cr.family("data", p, n, J, dtype)
    if c["far"]:
        # |mean| / spread = 1e2 and no centring at all: B grows with the shift's distance, and the bound must still hold
        rd = lambda a: a.astype(np.dtype(dtype)).astype(np.float64)                                  # noqa: E731
        d["U0"] = rd(d["U0"] - d["U0"].mean(axis=1, keepdims=True) + 100.0 * d["U0"].std(axis=1, keepdims=True))
        d["G"] = rd(d["G"] - d["G"].mean(axis=1, keepdims=True) + 100.0 * d["G"].std(axis=1, keepdims=True))
    eng = eng_mod.Engine(p, n, J, dtype=dtype, seed=SEED)
    eng.set_problem(d["y"], d["Gamma"], d["mu"], d["sigma"], d["ustar"])
    guards, U, G, _, _ = buffers(eng, d, c["shift"])
    sums = eng.colsum(U, G)
    sums_h = sums.cpu().numpy()
    rows = np.concatenate([d["U0"], d["G"]])
    assert sums_h[0] == J
    assert np.all(np.abs(sums_h[1:] - rows.sum(axis=1)) <= (J + 4) * cr.EPS["float64"] * np.abs(rows).sum(axis=1)), (label, "colsum")
    if c["far"]:
        sums = torch.zeros_like(sums)
        sums[0] = 1.0
        sums_h = sums.cpu().numpy()
    eng.set_shift(sums)
    shift = cr.round_shift(sums_h, dtype)
    mom = eng.moments(U, G)
    torch.cuda.synchronize()
    mom_h = mom.cpu().numpy()
    ref, scale = cr.moments_ref(d["U0"], d["G"], shift[:p], shift[p:])
    assert mom_h[0] == J
    cus = torch.cuda.get_device_properties(eng.device).multi_processor_count
    chain = cr.gram_chain(p, n, J, dtype, cus, gram_plan(p, n, J, dtype))
    arms = "+".join(sorted({arm for _, arm, _ in k1_launches(c, cus)}))
    held(mom_h[1:len(ref)], ref[1:], scale[1:], cr.c_gram(chain), eps, label, "K1 %s %s" % (arms, dtype) + ("/far" if c["far"] else ""))
    both = torch.full_like(mom, float("nan"))
    eng.moments_uu(U, G, out=both)
    eng.moments_rest(U, G, both)
    torch.cuda.synchronize()
    assert np.array_equal(both.cpu().numpy()[:len(ref)].view(np.uint64), mom_h[:len(ref)].view(np.uint64)), (label, "uu + rest != moments")
    if guards:
        for f, v in guards[:2]:
            assert guards_intact(f, v), (label, "written outside a buffer")
    eng.close()


@gpu
@pytest.mark.parametrize("c", K2_CASES, ids=k2_id)
def test_dense_algebra_from_the_devices_own_moments(eng_mod, c):
    """K2 (fp64 whatever the engine dtype) from the moment buffer THE DEVICE produced: ubar, gbar, C, K, M, hk, t, bias, self_bias
    at BAND = 1e-9 relative to each array's maximum, for both engine dtypes; L against numpy's Cholesky factor of the device's
    own C (potrf_reg_kernel up to p = 256, the blocked route above).  This is the stage that holds J - 1 against J and the 1e-8
    jitter: both are far below fp32 rounding of U_next and cannot be K3's business."""
    import torch
    p, n, J, dtype, upd = c["p"], c["n"], c["J"], c["dtype"], c["update"]
    label = k2_id(c)
    d = cr.family(c["fam"], p, n, J, dtype, dense_gamma=c["dg"], dense_sigma=c["ds"])
    kw, t_prev = TS_RULES[c["rule"]]
    eng = eng_mod.Engine(p, n, J, dtype=dtype, seed=SEED)
    eng.set_problem(d["y"], d["Gamma"], d["mu"], d["sigma"], d["ustar"])
    _, U, G, xi_t, out = buffers(eng, d, 0)
    sums = eng.colsum(U, G)
    eng.set_shift(sums)
    sums_h = sums.cpu().numpy().copy()
    Lg, Li = cr.whitening(d["Gamma"])
    if Lg is not None:                       # the engine centres the whitened rows: sums_g <- L^{-1} sums_g (whiten_sums_kernel)
        sums_h[1 + p:] = Li @ sums_h[1 + p:]
    shift = cr.round_shift(sums_h, dtype)
    mom = eng.moments(U, G)
    prm = eng_mod.step_params(update=upd, time_step=kw["time_step"], first_step=not t_prev, t_len=len(t_prev),
                              t_last=t_prev[-1] if t_prev else 0.0, delta_t=kw.get("delta_t"), spinup=kw.get("spinup", 4.0), T=30)
    if upd == "aldi_constant":
        eng.apply_drift(prm, mom, U, G, out)
        torch.cuda.synchronize()
    else:
        eng.apply(prm, mom, U, G, xi_t, out=out)
        res = eng.result()
    dd = eng.debug_dense()
    ref = cr.dense_ref(mom.cpu().numpy(), shift, d, upd, time_step=kw["time_step"], delta_t=kw.get("delta_t"),
                       spinup=kw.get("spinup", 4.0), first_step=not t_prev, t_len=len(t_prev), t_last=t_prev[-1] if t_prev else 0.0)
    worst = 0.0
    for key in ("ubar", "gbar", "C", "K", "M"):
        e = float(np.max(np.abs(dd[key] - ref[key])) / np.max(np.abs(ref[key])))
        worst = max(worst, e)
        assert e <= cr.BAND, (label, key, e)
    Lref = np.linalg.cholesky(dd["C"])
    e = float(np.max(np.abs(np.tril(dd["L"]) - Lref)) / np.max(np.abs(Lref)))
    assert e <= cr.BAND, (label, "L", e)
    worst = max(worst, e)
    if upd != "aldi_constant":
        for key, got in (("hk", res.hk), ("t", res.t_new), ("bias", res.bias), ("self_bias", res.self_bias)):
            e = abs(got - ref[key]) / abs(ref[key])
            worst = max(worst, e)
            assert e <= cr.BAND, (label, key, got, ref[key])
        if kw["time_step"] == "spectral":
            assert res.radspec == pytest.approx(ref["radspec"], rel=cr.BAND)
    note("K2 %s" % dtype, 0, worst / cr.BAND)
    eng.close()
