"""CPU check of the finisher's parked s_min queries under the wave's work budget (csrc/bvh_trace.h
bvh4_query_budget, WF_BVH_BUDGET), by tests/native/trip_budget_check.cpp: the budgeted wave loop restated on
the host (csrc/host/trace_host.h wave_call_budget) over waves of 64 lanes that take a new ray whenever their
query ends, for the budgets 1, 2, 3 and the shipped one:

* every lane's (s_min, tk) equals the unparked sequential query's (bvh4_smin) bit for bit;
* every query ends;
* no query takes more calls than it has bodies of its own (the progress rule: an unfinished lane executes at
  least one body in every call) — which is what makes a budget-1 run on the GPU safe to start.

20,000 seeded rays per scene: camera rays, bounces (grazing, axis-parallel), rays that start on the transparent
objects and rays that start 1e-4 off a triangle.  The GPU kernel: tests/test_gpu_query_budget.py.
"""
import os
import re
import subprocess

import pytest

import helpers

RAYS = 20_000


def shipped_budget():
    src = open(os.path.join(helpers.ROOT, "isaklm-raytracer_amd", "csrc", "wf_state.h")).read()
    return int(re.search(r"^#define WF_BVH_BUDGET (\d+)", src, re.M).group(1))


@pytest.fixture(scope="module")
def budget_check(tmp_path_factory):
    return helpers.build_native(tmp_path_factory.mktemp("trip"), "trip_budget_check")


def _field(line, name):
    return int(line.split(name + " ")[1].split()[0])


@pytest.mark.parametrize("name", ["cornell", "cornell_blob", "room_small"])
def test_budgeted_queries_equal_the_unparked_query_and_progress(budget_check, name):
    budgets = [1, 2, 3, shipped_budget()]
    assert budgets[3] >= 1
    r = subprocess.run([budget_check, helpers.scene_path(name), str(RAYS), "11"] + [str(b) for b in budgets],
                       capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    head = r.stdout.splitlines()[0]
    assert _field(head, "rays") == RAYS and _field(head, "off a triangle") > RAYS // 8, head
    if name == "room_small":  # (the room holds the two glass spheres; the Cornell boxes have no transparent object)
        assert _field(head, "on glass") > RAYS // 8, head
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("budget ")]
    assert [_field(ln, "budget") for ln in lines] == budgets, r.stdout
    for ln in lines:
        assert _field(ln, "queries") == RAYS, ln
        assert _field(ln, "mismatches") == 0 and _field(ln, "slow") == 0 and _field(ln, "unfinished") == 0, ln
    # the small budgets do park lanes in front of leaf visits (the state the old rule never had)
    assert _field(lines[0], "parks at a leaf") > 0, lines[0]
