"""The chain-summary kernels' rows of the register and scratch table (tools/isa_audit.py; no GPU needed): chain_half_kernel
carries a chain's shift and its four half sums for CS_RB rows in one lane's registers through a whole launch, and
chain_pool_kernel holds the next tile's loads, the rows' shifts and row sums and four MFMA accumulators at once -- nothing
may go to scratch and nothing may be spilled, in either engine dtype, and the pooled kernel's MFMAs sit in its loop.  The
counts are recorded in profiles/chainsum_isa_audit.txt."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

KERNELS = ["chain_half_kernel<double>", "chain_half_kernel<float>", "chain_pool_kernel<double>", "chain_pool_kernel<float>",
           "chain_pool_reduce_kernel", "chain_half_reduce_kernel", "chain_half_final_kernel", "chain_c_final_kernel"]


@pytest.fixture(scope="module")
def table():
    import isa_audit
    from ces_amd import build
    assert "kernels_chainsum.hip" in build.SOURCES         # (the table of `python tools/isa_audit.py` lists it)
    t = isa_audit.collect(["kernels_chainsum.hip"])
    names = isa_audit.demangle(sorted(t))
    return {re.sub(r"\(.*", "", names[k]).replace("cesx::", "").replace("void ", ""): v for k, v in t.items()}


def test_the_chain_summary_kernels_have_no_scratch_and_no_spills(table):
    assert sorted(table) == sorted(KERNELS)
    for name, r in table.items():
        assert r["ScratchSize [bytes/lane]"] == 0 and r["scratch_total"] == 0, name
        assert r["SGPRs Spill"] == 0 and r["VGPRs Spill"] == 0 and r["spill_total"] == 0 and r["spill_in_loop"] == 0, name


def test_the_pooled_kernel_runs_on_the_matrix_pipe(table):
    for t in ("double", "float"):
        r = table["chain_pool_kernel<%s>" % t]
        assert r["mfma"] == r["mfma_in_loop"] == 32, (t, r["mfma"], r["mfma_in_loop"])       # 8 k-steps x 4 accumulators per tile
        assert r["LDS Size [bytes/block]"] == 2 * 64 * 36 * 8
