"""gp_proj_coef_kernel's rows of the register and scratch table (tools/isa_audit.py; no GPU needed): a sub-wave group of lanes per
chain holds one row (two for 64 < k <= 128) of the factor's column, of a, z, e and h in registers -- nothing may go to scratch,
nothing may be spilled, the fp64 work stays on the vector ALU (no MFMA: the chains' matrices are k x k and triangular), and all
of its LDS is the dynamic region of gp_proj_lds(k) bytes (no static array in front of the groups' slices).  The table is
recorded in profiles/gpprojgrad_isa_audit.txt."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

INSTANCES = ["gp_proj_coef_kernel<%s>" % gs for gs in ("16, 1", "32, 1", "64, 1", "64, 2")]


@pytest.fixture(scope="module")
def table():
    import isa_audit
    from ces_amd import build
    assert "kernels_gpprojgrad.hip" in build.SOURCES       # (the table of `python tools/isa_audit.py` lists it)
    t = isa_audit.collect(["kernels_gpprojgrad.hip"])
    names = isa_audit.demangle(sorted(t))
    return {re.sub(r"\(.*", "", names[k]).replace("cesx::", "").replace("void ", ""): v for k, v in t.items()}


def test_the_coefficient_kernels_have_no_scratch_no_spills_no_mfma_and_no_static_lds(table):
    assert sorted(table) == sorted(INSTANCES)
    for name, r in table.items():
        assert r["ScratchSize [bytes/lane]"] == 0 and r["scratch_total"] == 0 and r["scratch_in_loop"] == 0, name
        assert r["SGPRs Spill"] == 0 and r["VGPRs Spill"] == 0 and r["spill_total"] == 0 and r["spill_in_loop"] == 0, name
        assert r["mfma"] == 0 and r["mfma_in_loop"] == 0, name
        assert r["LDS Size [bytes/block]"] == 0, name      # static LDS: none
        assert r["Occupancy [waves/SIMD]"] >= 4, name      # (LDS, not registers, decides how many chains a CU holds)


def test_the_table_is_on_record(table):
    with open(os.path.join(ROOT, "profiles", "gpprojgrad_isa_audit.txt")) as fh:
        text = fh.read()
    for name in INSTANCES:
        assert name in text, name
