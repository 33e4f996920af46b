"""The rows of the Darcy chain kernels in the register and scratch table (tools/isa_audit.py; no GPU needed): the four dc_*
kernels of kernels_darcy_chain.hip -- start, Langevin accept, leap, leapfrog accept; the last two in both ADAPT forms -- in both
engine dtypes.  A chain's vectors live in LDS, so nothing may go to scratch and nothing may be spilled; the products are on the
vector ALU (no MFMA: one wave's rows, fp64 sums in a fixed order); and the static LDS of a workgroup leaves room for at least two
per CU.  The counts are recorded in profiles/darcychain_isa_audit.txt."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

KERNELS = (["dc_start_kernel<%s>" % t for t in ("double", "float")]
           + ["dc_lv_accept_kernel<%s>" % t for t in ("double", "float")]
           + ["dc_hm_%s_kernel<%s, %s>" % (k, t, a) for k in ("leap", "accept") for t in ("double", "float") for a in ("true", "false")])
LDS_CU = 160 * 1024


@pytest.fixture(scope="module")
def table():
    import isa_audit
    from ces_amd import build
    assert "kernels_darcy_chain.hip" in build.SOURCES      # (the table of `python tools/isa_audit.py` lists it)
    t = isa_audit.collect(["kernels_darcy_chain.hip"])
    names = isa_audit.demangle(sorted(t))
    return {re.sub(r"\(.*", "", names[k]).replace("cesx::", "").replace("void ", ""): v for k, v in t.items()}


def test_the_kernel_set(table):
    assert sorted(table) == sorted(KERNELS) and len(KERNELS) == 12


def test_no_scratch_no_spills_no_mfma_and_two_workgroups_per_cu(table):
    for name, r in table.items():
        assert r["ScratchSize [bytes/lane]"] == 0 and r["scratch_total"] == 0, name
        assert r["SGPRs Spill"] == 0 and r["VGPRs Spill"] == 0 and r["spill_total"] == 0 and r["spill_in_loop"] == 0, name
        assert r["mfma"] == 0, name
        assert 0 < r["LDS Size [bytes/block]"] <= LDS_CU // 2, name
