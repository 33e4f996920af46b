"""The fused Langevin kernel's and the Jacobian kernel's rows of the register and scratch table (tools/isa_audit.py; no GPU
needed): a chain -- its state, phi, the counter, its g, the proposal with its map, Jacobian, grad phi and g, the Philox block
and the fp64 Box-Muller pair -- lives in one lane's registers for a whole launch, and the problem arrives by value in scalar
registers: nothing may go to scratch and nothing may be spilled, in either map instantiation, either engine dtype and each of
the four forms of the problem (a diagonal or a dense Gamma, a diagonal or a dense prior: the kernel's third parameter).  The
counts are recorded in profiles/mapgrad_isa_audit.txt."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

PAIRS = [(t, m) for t in ("double", "float") for m in ("MapElliptic", "MapBanana")]
FUSED = ["mh_langevin_map_kernel<%s, %s, %d>" % (tm + (dense,)) for tm in PAIRS for dense in range(4)]
JAC = ["map_jac_kernel<%s, %s>" % tm for tm in PAIRS]


@pytest.fixture(scope="module")
def table():
    import isa_audit
    from ces_amd import build
    assert "kernels_maps.hip" in build.SOURCES             # (the table of `python tools/isa_audit.py` lists it)
    t = isa_audit.collect(["kernels_maps.hip"])
    names = isa_audit.demangle(sorted(t))
    return {re.sub(r"\(.*", "", names[k]).replace("cesx::", "").replace("void ", ""): v for k, v in t.items()}


def test_the_langevin_and_jacobian_kernels_have_no_scratch_and_no_spills(table):
    rows = {k: v for k, v in table.items() if k.startswith(("mh_langevin_map_kernel<", "map_jac_kernel<"))}
    assert sorted(rows) == sorted(FUSED + JAC)
    for name, r in rows.items():
        assert r["ScratchSize [bytes/lane]"] == 0 and r["scratch_total"] == 0, name
        assert r["SGPRs Spill"] == 0 and r["VGPRs Spill"] == 0 and r["spill_total"] == 0 and r["spill_in_loop"] == 0, name
