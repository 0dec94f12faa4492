"""CPU check of wf_check's launch shape (csrc/wf_check_grid.h, DESIGN.md §5
"Run-time guard"), by tests/native/check_grid_check.cpp: for record estimates
of 0, 1, one block, the record buffer's capacity and beyond, the grid stays
within [WF_CHECK_BLOCKS, spill_threads / WF_BLOCK]; a chained call's is
WF_CHECK_BLOCKS; an unchained call's is a lane per record between those
bounds.  The GPU side is tests/test_gpu_guard_shape.py."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "isaklm-raytracer_amd", "csrc")
BLOCK, MIN_BLOCKS = 256, 256


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("grid") / "check_grid_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + CSRC,
                    os.path.join(ROOT, "tests", "native", "check_grid_check.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "out of bounds 0\n" in r.stdout and "small 100 100\n" in r.stdout, r.stdout
    rows = [[int(v) for v in ln.replace("->", "").split()[1:]] for ln in r.stdout.splitlines() if ln.startswith("grid ")]
    assert len(rows) == 3 * 4 * 13 * 2
    return rows


def test_grid_stays_within_its_bounds(cases):
    for chained, want, cap, spill, g in cases:
        assert MIN_BLOCKS <= g <= spill // BLOCK, (chained, want, cap, spill, g)


def test_chained_calls_keep_the_small_grid(cases):
    assert all(g == MIN_BLOCKS for chained, _, _, _, g in cases if chained)


def test_unchained_grid_is_a_lane_per_record(cases):
    for chained, want, cap, spill, g in cases:
        if not chained:
            need = -(-min(want, cap) // BLOCK)  # ceil
            assert g == min(max(need, MIN_BLOCKS), spill // BLOCK), (want, cap, spill, g)
    # the bench's call (about 1.04 M records estimated, 2^20 capacity, 1,024 blocks of spill lanes): the whole area
    assert any(not c and w == 1 << 20 and cap == 1 << 20 and s == 1024 * BLOCK and g == 1024
               for c, w, cap, s, g in cases)
