"""The lagged-sum kernels' rows of the register and scratch table (tools/isa_audit.py; no GPU needed): chain_acf_kernel holds
P_0 .. P_LT and -- LT = 8 and 32 -- the ring of the last LT values in one lane's registers, or -- LT = 64 -- the ring in static
LDS, 64 slots x 64 lanes x 8 bytes; nothing may go to scratch and nothing may be spilled, in either engine dtype and in any
instantiation.  The static LDS stays within the budget DESIGN.md section 5o states: 32 KiB for the LDS ring, the 2 KiB of
the reduce's tree, none elsewhere.  The counts are recorded in profiles/chainacf_isa_audit.txt."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

LAG = ["chain_acf_kernel<%s, %s>" % (t, v) for t in ("double", "float") for v in ("8, false", "32, false", "64, true")]
KERNELS = LAG + ["chain_acf_pack_kernel<double>", "chain_acf_pack_kernel<float>", "chain_acf_final_kernel", "chain_acf_reduce_kernel"]
LDS_BUDGET = {"64, true": 64 * 64 * 8, "reduce": 256 * 8}


@pytest.fixture(scope="module")
def table():
    import isa_audit
    from ces_amd import build
    assert "kernels_chainacf.hip" in build.SOURCES          # (the table of `python tools/isa_audit.py` lists it)
    t = isa_audit.collect(["kernels_chainacf.hip"])
    names = isa_audit.demangle(sorted(t))
    return {re.sub(r"\(.*", "", names[k]).replace("cesx::", "").replace("void ", ""): v for k, v in t.items()}


def test_the_lagged_sum_kernels_have_no_scratch_and_no_spills(table):
    assert sorted(table) == sorted(KERNELS)
    for name, r in table.items():
        assert r["ScratchSize [bytes/lane]"] == 0 and r["scratch_total"] == 0, name
        assert r["SGPRs Spill"] == 0 and r["VGPRs Spill"] == 0 and r["spill_total"] == 0 and r["spill_in_loop"] == 0, name


def test_static_lds_is_within_the_stated_budget(table):
    for name, r in table.items():
        if name.endswith("64, true>"):
            assert 0 < r["LDS Size [bytes/block]"] <= LDS_BUDGET["64, true"], (name, r["LDS Size [bytes/block]"])
        elif name == "chain_acf_reduce_kernel":
            assert 0 < r["LDS Size [bytes/block]"] <= LDS_BUDGET["reduce"], (name, r["LDS Size [bytes/block]"])
        else:
            assert r["LDS Size [bytes/block]"] <= 8, (name, r["LDS Size [bytes/block]"])      # (the unused ring's one double, if kept)
