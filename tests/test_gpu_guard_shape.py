"""The launch shape of the run-time guard's re-trace (wf_check; DESIGN.md §5
"Run-time guard", csrc/wf_check_grid.h).

A chained call's wf_check runs beside the next call's finisher on 256 blocks.
An unchained call's runs alone on the chip, inside the caller's wait, and gets
a lane per record it may hold, up to the lanes of the stack spill area (the
finisher's grid: CUs x 4 SIMDs x 4 waves / 4 waves per block, 256 lanes each).
The guard itself must not notice: the same records, the same comparisons.

Every render here is the wavefront kernel with the bounded traversal and
check_interval=1: every finisher ray is recorded, whatever call it runs in, so
the record counts of an unchained call and of chained calls compare.  The
"chained" renders pass overlap=True and launch every call (coalesce_passes
< 0): each of their checks takes the 256-block grid, the chain's first call
included.

Where counts are compared, the deep-path hand-off is off (wf_long_depth < 0):
every ray of a pixel is then a ray of its call's finisher.  With the hand-off
on, a pixel wf_long gives back after its chained call's finisher has ended
runs on in the chain's drain, which records nothing (launch_drain: no guard
records), so a chained render's count falls short of the unchained one's by
the drain's rays, a few and not the same from run to run (room_small 256 x 256
x 8: 1,856,859 unchained against 1,856,845 chained).  The first test renders
the default hand-off too, unchained, and holds it to the same frame.
"""
import ctypes

import numpy as np
import pytest

import helpers
import rt

pytestmark = pytest.mark.gpu
WF = rt.KERNEL_WAVEFRONT
WF_BLOCK = 256


def _spill_lanes():
    """the most lanes wf_check's grid may have: the finisher's grid, as launch_whole_now sizes the spill area"""
    hip = ctypes.CDLL("libamdhip64.so")
    cus = ctypes.c_int(0)
    assert hip.hipDeviceGetAttribute(ctypes.byref(cus), 63, 0) == 0  # hipDeviceAttributeMultiprocessorCount
    assert 1 <= cus.value <= 4096, cus.value
    return cus.value * 4 * 4 // (WF_BLOCK // 64) * WF_BLOCK


def _render(run, W, H, passes, chained, debug=0, wf_long_depth=-1):
    """(G-buffer arrays, deviation block) of one guarded render; passes: one entry per call;
    wf_long_depth < 0: no hand-off to wf_long (0: the default depth)"""
    rt.join()
    rt.deviation_stats(reset=True)
    out, _, _ = run.render(W, H, passes, kernel=WF, traversal=rt.TRAVERSAL_BOUNDED, check_interval=1,
                           overlap=chained, debug=debug, coalesce_passes=-1, wf_long_depth=wf_long_depth)
    dev = rt.deviation_stats(reset=True)
    print("chained" if chained else "unchained", W, H, passes, "checked", dev["bounded_checked"], "mismatches",
          dev["bounded_mismatches"], "dropped", dev["check_dropped"])
    return out, dev


def test_several_rounds_and_the_last_rounds_tail():
    run = helpers.GpuRun("room_small")
    W, H = 256, 256
    one, d1 = _render(run, W, H, [8], chained=False)
    two, d2 = _render(run, W, H, [4, 4], chained=True)
    lanes = _spill_lanes()
    print("lanes of the enlarged grid", lanes)
    # more records than the enlarged grid has lanes: a second round runs, and its last wave is partly empty
    assert d1["bounded_checked"] > lanes and d1["bounded_checked"] % lanes != 0, (d1, lanes)
    assert d1["bounded_checked"] >= W * H * 8, d1  # at least the camera rays
    for d in (d1, d2):
        assert d["bounded_mismatches"] == 0 and d["check_dropped"] == 0, d
    assert d1["bounded_checked"] == d2["bounded_checked"], (d1, d2)
    helpers.assert_bitwise(two, one, what="two chained 4-pass calls vs one unchained 8-pass call")
    ref, _ = helpers.oracle_render(run.path, W, H, [8])
    helpers.assert_bitwise(one, ref, what="room_small 256x256x8, guard on every ray")
    # the default hand-off depth: deep paths leave for wf_long (their rays past the hand-off are not the finisher's)
    deep, d3 = _render(run, W, H, [8], chained=False, wf_long_depth=0)
    assert lanes < d3["bounded_checked"] <= d1["bounded_checked"], (d3, d1)
    assert d3["bounded_mismatches"] == 0 and d3["check_dropped"] == 0, d3
    helpers.assert_bitwise(deep, ref, what="room_small 256x256x8, guard on every ray, deep paths in wf_long")


def test_fewer_records_than_one_wave():
    run = helpers.GpuRun("cornell")
    one, d1 = _render(run, 8, 8, [1], chained=False)
    ch, d2 = _render(run, 8, 8, [1], chained=True)
    assert d1["bounded_checked"] >= 1 and d1["bounded_checked"] == d2["bounded_checked"], (d1, d2)
    for d in (d1, d2):
        assert d["bounded_mismatches"] == 0 and d["check_dropped"] == 0, d
    helpers.assert_bitwise(ch, one, what="8x8x1 chained vs unchained")


def test_the_enlarged_grid_really_compares():
    """RT_DEBUG_CHECK_FAULT (debug=4) writes a wrong result into every record: the re-trace must flag
    each of them, on either grid."""
    run = helpers.GpuRun("cornell")
    _, d1 = _render(run, 128, 128, [4], chained=False, debug=rt.DEBUG_CHECK_FAULT)
    _, d2 = _render(run, 128, 128, [4], chained=True, debug=rt.DEBUG_CHECK_FAULT)
    assert d1["bounded_mismatches"] > 0, d1
    assert d1["bounded_mismatches"] == d2["bounded_mismatches"], (d1, d2)
    assert d1["bounded_mismatches"] == d1["bounded_checked"] == d2["bounded_checked"], (d1, d2)
    assert d1["check_dropped"] == 0 and d2["check_dropped"] == 0, (d1, d2)
    assert np.any(np.asarray(d1["mismatch_ray"]) != 0.0), d1
