"""CPU check of wf_check's launch shape (csrc/wf_check_grid.h, DESIGN.md §5
"Run-time guard"), by tests/native/check_grid_check.cpp: for record estimates
of 0, 1, one block, the record buffer's capacity and beyond, the grid stays
within [WF_CHECK_BLOCKS, spill_threads / WF_BLOCK]; a chained call's is
WF_CHECK_BLOCKS; an unchained call's is a lane per record between those
bounds; and the record estimate and capacity that grid and the record buffer are
sized from (wf_check_records) equal launch_whole_now's former expressions,
written out here.  The GPU side is tests/test_gpu_guard_shape.py."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "isaklm-raytracer_amd", "csrc")
BLOCK, MIN_BLOCKS = 256, 256


@pytest.fixture(scope="module")
def output(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("grid") / "check_grid_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + CSRC,
                    os.path.join(ROOT, "tests", "native", "check_grid_check.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "out of bounds 0\n" in r.stdout and "small 100 100\n" in r.stdout, r.stdout
    return r.stdout


def _rows(output, tag):
    return [[int(v) for v in ln.replace("->", "").split()[1:]] for ln in output.splitlines() if ln.startswith(tag + " ")]


@pytest.fixture(scope="module")
def cases(output):
    rows = _rows(output, "grid")
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


def test_record_estimate_and_capacity(output):
    """wf_check_records against the expressions launch_whole_now held: per sample 2 * depth + 2 rays when every
    ray is recorded (depth: wf_long_depth, 64 by default), 8 otherwise; want = pixels * passes * per sample /
    interval; the capacity doubles from 2^16 while below want, up to 2^22.  Expected figures by hand."""
    def former(slots, passes, mask, long_depth):
        if mask == 0xFFFFFFFF:
            return 0, 0
        per_sample = 2 * (long_depth if long_depth > 0 else 64) + 2 if mask == 0 else 8
        want = slots * passes * per_sample // (mask + 1)
        cap = 1 << 16
        while cap < want and cap < (1 << 22):
            cap <<= 1
        return cap, want

    by_hand = {
        (1920 * 1080, 64, 4095, 0): (1 << 18, 259200),                 # 2,073,600 * 64 * 8 / 4,096
        (48 * 27, 3, 0, 0): (1 << 19, 505440),                         # 1,296 * 3 * 130
        (48 * 27, 3, 0, 16): (1 << 18, 132192),                        # 1,296 * 3 * 34
        (1920 * 1080, 1024, 0, 0): (1 << 22, 2073600 * 1024 * 130),    # saturates WF_CHECK_CAP
        (1920 * 1080, 64, 0xFFFFFFFF, 0): (0, 0),                      # the guard off
    }
    rows = _rows(output, "records")
    assert len(rows) == len(by_hand)
    for slots, passes, mask, long_depth, cap, want in rows:
        assert (cap, want) == by_hand[(slots, passes, mask, long_depth)], (slots, passes, mask, long_depth, cap, want)
        assert (cap, want) == former(slots, passes, mask, long_depth)
