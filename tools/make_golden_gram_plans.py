"""Writes tests/golden/gram_plan_info.json: the six info integers of cesx_debug_gram_plan (types, workgroups, blocks,
busiest workgroup's tiles x blocks-per-SIMD, max staged row blocks, slabs) for every case of the sweep of
tests/test_abi.py::test_gram_work_partition_invariants.  Host only.

    python tools/make_golden_gram_plans.py [path of libcesx.so]

The fixture pins the planner across refactors: it is written from the library of the commit a change STARTS from and
is not regenerated from the changed tree (tests/test_gram_plans_host.py).
"""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(256, 256), (2, 2), (10, 6), (33, 17), (64, 50), (96, 80), (300, 40), (40, 300), (250, 250), (512, 512),
          (700, 96), (130, 520)]
DTYPES = [0, 1]
JS = [32, 1004, 4096, 65536, 524288]
BUDGETS = [256, 248, 224, 64, 3]
PARTS = [0, 1]


def sweep():
    for p, n in SHAPES:
        for dtype in DTYPES:
            for J in JS:
                for budget in BUDGETS:
                    for part in PARTS:
                        yield p, n, dtype, J, budget, part


def main():
    lib = ctypes.CDLL(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "ces_amd", "libcesx.so"))
    lib.cesx_debug_gram_plan.argtypes = [ctypes.c_int] * 5 + [ctypes.c_longlong, ctypes.POINTER(ctypes.c_int)]
    info = (ctypes.c_int * 6)()
    rows = []
    for p, n, dtype, J, budget, part in sweep():
        assert lib.cesx_debug_gram_plan(p, n, dtype, part, budget, J, info) == 0, (p, n, dtype, J, budget, part)
        rows.append(list(info))
    head = {"shapes": SHAPES, "dtypes": DTYPES, "J": JS, "budgets": BUDGETS, "parts": PARTS}
    path = os.path.join(ROOT, "tests", "golden", "gram_plan_info.json")
    with open(path, "w") as f:      # one line per (shape, dtype, J): the 5 budgets x 2 parts of it
        f.write("{" + ", ".join('"%s": %s' % (k, json.dumps(v)) for k, v in head.items()) + ',\n "info": [\n')
        per = len(BUDGETS) * len(PARTS)
        lines = [", ".join(json.dumps(r, separators=(",", ":")) for r in rows[i:i + per]) for i in range(0, len(rows), per)]
        f.write(",\n".join("  " + ln for ln in lines) + "\n ]}\n")
    print(path, len(rows), "cases", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
