"""The GP-gradient and Langevin kernels' rows of the register and scratch table (tools/isa_audit.py; no GPU needed):
gp_grad_kernel holds one tile's scalars and two MFMA accumulator pairs, the lv_* kernels a chain's running sums -- nothing may
go to scratch and nothing may be spilled, in either engine dtype and on either side of the LDS boundary.  The matrix pipe is
used by the gradient kernel alone (its variance phases: W = L^{-1} K* and beta = L^{-T} W; the mean-only mode is the same
kernel with both skipped).  The counts are recorded in profiles/gpgrad_isa_audit.txt."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

GRAD = ["gp_grad_kernel<%s, %s>" % (t, l) for t in ("double", "float") for l in ("true", "false")]
STEP = ["lv_%s_kernel<%s>" % (k, t) for k in ("start", "propose", "accept") for t in ("double", "float")]


@pytest.fixture(scope="module")
def table():
    import isa_audit
    from ces_amd import build
    assert "kernels_gpgrad.hip" in build.SOURCES           # (the table of `python tools/isa_audit.py` lists it)
    t = isa_audit.collect(["kernels_gpgrad.hip"])
    names = isa_audit.demangle(sorted(t))
    return {re.sub(r"\(.*", "", names[k]).replace("cesx::", "").replace("void ", ""): v for k, v in t.items()}


def test_the_gradient_and_langevin_kernels_have_no_scratch_and_no_spills(table):
    assert sorted(table) == sorted(GRAD + STEP)
    for name, r in table.items():
        assert r["ScratchSize [bytes/lane]"] == 0 and r["scratch_total"] == 0, name
        assert r["SGPRs Spill"] == 0 and r["VGPRs Spill"] == 0 and r["spill_total"] == 0 and r["spill_in_loop"] == 0, name


def test_the_matrix_pipe_is_the_gradient_kernels(table):
    for name in GRAD:
        assert table[name]["mfma"] > 0 and table[name]["mfma_in_loop"] == table[name]["mfma"], name
        assert table[name]["LDS Size [bytes/block]"] == 8192, name      # the partial sums; the tile is dynamic LDS
    for name in STEP:
        assert table[name]["mfma"] == 0 and table[name]["LDS Size [bytes/block]"] == 0, name
