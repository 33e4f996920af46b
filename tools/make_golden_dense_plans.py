"""Writes tests/golden/dense_plan.json: the K2 plans (plan_dense, 23 facts -> 13 fields, include/cesx.h) of the sweep of
tests/test_dense_plans_host.py, as one digest per group, and the 16 plans of the benchmark's engine state by name.  Host only.

    python tools/make_golden_dense_plans.py <dumper>

The fixture comes from the PARENT of the change that introduced plan_dense, never from a tree that has it: <dumper> is
tools/plan_dump.hip built in an export of that parent with a stand-in for cesx_debug_dense_plan in front of it (DENSE_PLAN_FN)
that holds the parent's launch_dense conditions, verbatim and in order, every launch replaced by a record of it.  A later change
of plan_dense that means to leave K2 alone regenerates it the same way: from the dumper of the commit it STARTS from.

Layout of `<dumper> dense sweep` (one line `facts : plan` per case): 256 groups of 1024 cases -- (update, phase) x time step x
dtype x diag_sigma x chain x p class, the factorial over the ten booleans the routes branch on -- then, for each of the six
single switches (hkfree_ok, update_v2, d_Wq, fuse_center_ok, fuse_center_auto, gram_b_short), 256 x 32 cases.  A digest is the
first 16 hex digits of the SHA-256 of a group's lines.
"""
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUPS, GROUP_CASES, SWITCHES, SWITCH_CASES = 256, 1024, 6, 256 * 32


def digest(lines):
    return hashlib.sha256("".join(lines).encode()).hexdigest()[:16]


def main():
    dumper = sys.argv[1]
    lines = subprocess.run([dumper, "dense", "sweep"], check=True, capture_output=True, text=True).stdout.splitlines(True)
    bench = subprocess.run([dumper, "dense", "bench"], check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(lines) == GROUPS * GROUP_CASES + SWITCHES * SWITCH_CASES and len(bench) == 16
    groups = [digest(lines[g * GROUP_CASES:(g + 1) * GROUP_CASES]) for g in range(GROUPS)]
    off = GROUPS * GROUP_CASES
    switches = [digest(lines[off + k * SWITCH_CASES:off + (k + 1) * SWITCH_CASES]) for k in range(SWITCHES)]
    path = os.path.join(ROOT, "tests", "golden", "dense_plan.json")
    with open(path, "w") as f:
        f.write('{"cases": %d, "sha256": "%s",\n "groups": [\n' % (len(lines), hashlib.sha256("".join(lines).encode()).hexdigest()))
        f.write(",\n".join("  " + ", ".join('"%s"' % d for d in groups[i:i + 8]) for i in range(0, GROUPS, 8)))
        f.write('\n ],\n "switches": %s,\n "bench": [\n' % json.dumps(switches))
        f.write(",\n".join("  " + json.dumps(b) for b in bench) + "\n ]}\n")
    print(path, len(lines), "cases", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
