"""The rows of the linear maps' Langevin kernels in the register and scratch table (tools/isa_audit.py; no GPU needed):
lvlin_accept_kernel keeps V chains' three fp64 sums and the loaded rows in a lane's registers, and the two element-wise kernels
one vector -- nothing may go to scratch and nothing may be spilled, in either engine dtype and either alignment form.  The
counts are recorded in profiles/lvlin_isa_audit.txt."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

ACCEPT = ["lvlin_accept_kernel<%s, %s>" % (t, v) for t in ("double", "float") for v in ("false", "true")]
ELEMENTWISE = ["%s<%s>" % (k, t) for k in ("lvlin_z_kernel", "lvlin_exph_kernel") for t in ("double", "float")]


@pytest.fixture(scope="module")
def table():
    import isa_audit
    from ces_amd import build
    assert "kernels_lvlin.hip" in build.SOURCES            # (the table of `python tools/isa_audit.py` lists it)
    t = isa_audit.collect(["kernels_lvlin.hip"])
    names = isa_audit.demangle(sorted(t))
    return {re.sub(r"\(.*", "", names[k]).replace("cesx::", "").replace("void ", ""): v for k, v in t.items()}


def test_the_lvlin_kernels_have_no_scratch_and_no_spills(table):
    rows = {k: v for k, v in table.items() if k.startswith("lvlin_")}
    assert sorted(rows) == sorted(ACCEPT + ELEMENTWISE)
    for name, r in rows.items():
        assert r["ScratchSize [bytes/lane]"] == 0 and r["scratch_total"] == 0, name
        assert r["SGPRs Spill"] == 0 and r["VGPRs Spill"] == 0 and r["spill_total"] == 0 and r["spill_in_loop"] == 0, name
