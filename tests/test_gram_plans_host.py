"""The Gram work partition, pinned: the plan fixes the order of the fp32 partial sums of both moments launches, so a change
of the planner's host code that means to leave the numbers alone has to leave every plan alone.  Host only (no device)."""
import ctypes
import json
import os

import pytest

from conftest import GOLDEN

# the sweep of tests/test_abi.py::test_gram_work_partition_invariants
SHAPES = [(256, 256), (2, 2), (10, 6), (33, 17), (64, 50), (96, 80), (300, 40), (40, 300), (250, 250), (512, 512),
          (700, 96), (130, 520)]
DTYPES = [0, 1]
JS = [32, 1004, 4096, 65536, 524288]
BUDGETS = [256, 248, 224, 64, 3]
PARTS = [0, 1]


@pytest.fixture(scope="module")
def lib():
    from ces_amd import build, engine
    build.build_lib()
    return engine.load_library()


def test_gram_plan_info_is_the_recorded_one(lib):
    """cesx_debug_gram_plan (min_types = 1, the caller's budget, no re-plan) gives, for every case of the sweep -- 12 shapes
    x 2 dtypes x 5 J x 5 budgets x 2 parts -- the six info integers {types, workgroups, blocks, busiest workgroup's tiles x
    blocks-per-SIMD, max staged row blocks, slabs} recorded in tests/golden/gram_plan_info.json
    (tools/make_golden_gram_plans.py, run on the commit BEFORE a change of the planner; never regenerated from the change)."""
    with open(os.path.join(GOLDEN, "gram_plan_info.json")) as fh:
        gold = json.load(fh)
    assert [tuple(s) for s in gold["shapes"]] == SHAPES and gold["dtypes"] == DTYPES and gold["J"] == JS
    assert gold["budgets"] == BUDGETS and gold["parts"] == PARTS
    want = iter(gold["info"])
    assert len(gold["info"]) == len(SHAPES) * len(DTYPES) * len(JS) * len(BUDGETS) * len(PARTS) == 1200
    info = (ctypes.c_int * 6)()
    for p, n in SHAPES:
        for dtype in DTYPES:
            for J in JS:
                for budget in BUDGETS:
                    for part in PARTS:
                        assert lib.cesx_debug_gram_plan(p, n, dtype, part, budget, J, info) == 0
                        assert list(info) == next(want), (p, n, dtype, J, budget, part)
