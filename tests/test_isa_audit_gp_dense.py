"""gp_score_dense_kernel's row of the register and scratch table (tools/isa_audit.py; no GPU needed): one wave per chain
holds two rows of the factor's column, two of d and the running sums in registers -- nothing may go to scratch, and all of
its LDS is the dynamic region (no static array in front of it: the packed factor starts 16-byte aligned)."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def table():
    import isa_audit
    from ces_amd import build
    assert "kernels_gpdense.hip" in build.SOURCES          # (the table of `python tools/isa_audit.py` lists it)
    t = isa_audit.collect(["kernels_gpdense.hip"])
    names = isa_audit.demangle(sorted(t))
    return {re.sub(r"\(.*", "", names[k]).replace("cesx::", "").replace("void ", ""): v for k, v in t.items()}


def test_the_dense_score_kernel_has_no_scratch_and_no_spills(table):
    rows = {k: v for k, v in table.items() if k.startswith("gp_score_dense_kernel<")}
    assert sorted(rows) == ["gp_score_dense_kernel<double>", "gp_score_dense_kernel<float>"]
    for name, r in rows.items():
        assert r["ScratchSize [bytes/lane]"] == 0 and r["scratch_total"] == 0, name
        assert r["SGPRs Spill"] == 0 and r["VGPRs Spill"] == 0 and r["spill_in_loop"] == 0, name
        assert r["LDS Size [bytes/block]"] == 0, name      # static LDS: none
        assert r["Occupancy [waves/SIMD]"] >= 4, name      # (LDS, not registers, decides how many chains a CU holds)
