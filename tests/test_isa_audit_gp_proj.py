"""gp_score_proj_kernel's rows of the register and scratch table (tools/isa_audit.py; no GPU needed): a sub-wave group of
lanes per chain holds one row (two for 64 < k <= 128) of the factor's column, of a and the running sums in registers --
nothing may go to scratch, and all of its LDS is the dynamic region (no static array in front of the groups' slices)."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

INSTANCES = ["gp_score_proj_kernel<%s, %s>" % (t, gs) for t in ("double", "float") for gs in ("16, 1", "32, 1", "64, 1", "64, 2")]


@pytest.fixture(scope="module")
def table():
    import isa_audit
    from ces_amd import build
    assert "kernels_gpproj.hip" in build.SOURCES           # (the table of `python tools/isa_audit.py` lists it)
    t = isa_audit.collect(["kernels_gpproj.hip"])
    names = isa_audit.demangle(sorted(t))
    return {re.sub(r"\(.*", "", names[k]).replace("cesx::", "").replace("void ", ""): v for k, v in t.items()}


def test_the_proj_score_kernels_have_no_scratch_no_spills_and_no_static_lds(table):
    rows = {k: v for k, v in table.items() if k.startswith("gp_score_proj_kernel<")}
    assert sorted(rows) == sorted(INSTANCES)
    for name, r in rows.items():
        assert r["ScratchSize [bytes/lane]"] == 0 and r["scratch_total"] == 0, name
        assert r["SGPRs Spill"] == 0 and r["VGPRs Spill"] == 0 and r["spill_in_loop"] == 0, name
        assert r["LDS Size [bytes/block]"] == 0, name      # static LDS: none
        assert r["Occupancy [waves/SIMD]"] >= 4, name      # (LDS, not registers, decides how many chains a CU holds)
