"""The chain-marginal kernels' rows of the register and scratch table (tools/isa_audit.py; no GPU needed): chain_hist1_kernel
holds CH_DU draws of CH_RB rows, the rows' range and each row's running bin and run length in one lane's registers, and
chain_hist2_kernel the two rows of a pair -- nothing may go to scratch and nothing may be spilled, in either engine dtype.
The counters live in static LDS: the 2-D kernel's is the bins2d = 64 table and the pair's two edge rows, nothing more (its
outside count stays in registers).  The counts are recorded in profiles/chainhist_isa_audit.txt."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

KERNELS = ["chain_hist1_kernel<double>", "chain_hist1_kernel<float>", "chain_hist2_kernel<double>", "chain_hist2_kernel<float>"]


@pytest.fixture(scope="module")
def table():
    import isa_audit
    from ces_amd import build
    assert "kernels_chainhist.hip" in build.SOURCES        # (the table of `python tools/isa_audit.py` lists it)
    t = isa_audit.collect(["kernels_chainhist.hip"])
    names = isa_audit.demangle(sorted(t))
    return {re.sub(r"\(.*", "", names[k]).replace("cesx::", "").replace("void ", ""): v for k, v in t.items()}


def test_the_chain_marginal_kernels_have_no_scratch_and_no_spills(table):
    assert sorted(table) == sorted(KERNELS)
    for name, r in table.items():
        assert r["ScratchSize [bytes/lane]"] == 0 and r["scratch_total"] == 0, name
        assert r["SGPRs Spill"] == 0 and r["VGPRs Spill"] == 0 and r["spill_total"] == 0 and r["spill_in_loop"] == 0, name
        assert r["mfma"] == 0, name                        # integer counting: nothing for the matrix pipe


def test_the_counters_are_in_static_lds(table):
    for t in ("double", "float"):
        r2 = table["chain_hist2_kernel<%s>" % t]
        assert 0 < r2["LDS Size [bytes/block]"] <= 64 * 64 * 4 + 2 * 65 * 8, (t, r2["LDS Size [bytes/block]"])
        r1 = table["chain_hist1_kernel<%s>" % t]           # CH_RB = 4 rows: B + 2 counters and B + 1 edges each at B = 256
        assert 0 < r1["LDS Size [bytes/block]"] <= 4 * (258 * 4 + 257 * 8), (t, r1["LDS Size [bytes/block]"])
