"""mh_run_map_kernel's rows of the register and scratch table (tools/isa_audit.py; no GPU needed): a chain -- its state, the
proposal, phi, the counter, the Philox block and the fp64 Box-Muller pair -- lives in one lane's registers for a whole
launch, and the problem arrives by value in scalar registers: nothing may go to scratch and nothing may be spilled, in
either map instantiation and either engine dtype.  The counts are recorded in profiles/maps_isa_audit.txt."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

INSTANCES = ["mh_run_map_kernel<%s, %s>" % (t, m) for t in ("double", "float") for m in ("MapElliptic", "MapBanana")]


@pytest.fixture(scope="module")
def table():
    import isa_audit
    from ces_amd import build
    assert "kernels_maps.hip" in build.SOURCES             # (the table of `python tools/isa_audit.py` lists it)
    t = isa_audit.collect(["kernels_maps.hip"])
    names = isa_audit.demangle(sorted(t))
    return {re.sub(r"\(.*", "", names[k]).replace("cesx::", "").replace("void ", ""): v for k, v in t.items()}


def test_the_fused_chain_kernels_have_no_scratch_and_no_spills(table):
    rows = {k: v for k, v in table.items() if k.startswith("mh_run_map_kernel<")}
    assert sorted(rows) == sorted(INSTANCES)
    for name, r in rows.items():
        assert r["ScratchSize [bytes/lane]"] == 0 and r["scratch_total"] == 0, name
        assert r["SGPRs Spill"] == 0 and r["VGPRs Spill"] == 0 and r["spill_total"] == 0 and r["spill_in_loop"] == 0, name
