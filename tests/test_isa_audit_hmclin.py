"""The rows of the linear maps' leapfrog kernels in the register and scratch table (tools/isa_audit.py; no GPU needed):
hl_accept_kernel keeps V chains' three fp64 sums and the loaded rows in a lane's registers, hl_kick_kernel one or two vectors --
nothing may go to scratch and nothing may be spilled, in either engine dtype, either alignment form, armed or not.  The counts
are recorded in profiles/hmclin_isa_audit.txt."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

ACCEPT = ["hl_accept_kernel<%s, %s, %s>" % (t, v, a) for t in ("double", "float") for v in ("false", "true") for a in ("false", "true")]
KICK = ["hl_kick_kernel<%s, %s>" % (t, a) for t in ("double", "float") for a in ("false", "true")]


@pytest.fixture(scope="module")
def table():
    import isa_audit
    from ces_amd import build
    assert "kernels_hmclin.hip" in build.SOURCES           # (the table of `python tools/isa_audit.py` lists it)
    t = isa_audit.collect(["kernels_hmclin.hip"])
    names = isa_audit.demangle(sorted(t))
    return {re.sub(r"\(.*", "", names[k]).replace("cesx::", "").replace("void ", ""): v for k, v in t.items()}


def test_the_hmclin_kernels_have_no_scratch_and_no_spills(table):
    rows = {k: v for k, v in table.items() if k.startswith("hl_")}
    assert sorted(rows) == sorted(ACCEPT + KICK)
    for name, r in rows.items():
        assert r["ScratchSize [bytes/lane]"] == 0 and r["scratch_total"] == 0, name
        assert r["SGPRs Spill"] == 0 and r["VGPRs Spill"] == 0 and r["spill_total"] == 0 and r["spill_in_loop"] == 0, name
