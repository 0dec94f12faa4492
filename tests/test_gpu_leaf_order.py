"""GPU frames of the finisher and wf_long as built with RT_COLD_ARGS (csrc/wf_state.h: the rare paths
read their state from the kernel's argument block where they use it), each compared bit for bit with
the oracle's, wavefront renderer, bounded traversal:

* Cornell, 64 x 64, 4 spp;
* the duplicated quad (every hit on it is a tie at equal s) and the adversarial "near" room,
  64 x 64, 2 spp;
* room_small 96 x 64, 2 spp, with the run-time guard on EVERY ray (check_interval=1: each finisher ray
  re-traced by the plain KD traversal): 0 mismatches, and every hand-off failure counter 0;
* the same frame as two chained calls (1 + 1 passes);
* room_small 96 x 64, 2 spp, aimed at its glass sphere (tests/test_gpu_deep_bounded.py's view) with
  wf_long_depth at its minimum (16), as one call and as 1 + 1 chained calls, the guard on every
  finisher ray.  The oracle's own paths of this frame go far past the hand-off depth (asserted: one of
  826 bounces), and the GPU's deviation block must show that deep path too, so the hand-off
  (publish_long_capped, long_publish), wf_long's claim, its return or release of the pixel and the
  finisher's return-ring claim — the paths whose reads moved — really run.

(The file's name is the one the issue that added it gave it, for its part A, the nearest-first leaf
scan; that part measured slower and is not in the tree, DESIGN.md §9.  These frames are RT_COLD_ARGS's.)
"""
import numpy as np
import pytest

import hazards
import helpers
import oracle
import rt

pytestmark = pytest.mark.gpu
WF = rt.KERNEL_WAVEFRONT
BOUNDED = dict(kernel=WF, traversal=rt.TRAVERSAL_BOUNDED)
LONG = 16  # the hand-off's minimum depth (wavefront.hip WF_LONG_DEPTH_MIN)
# every hand-off failure counter and the overflow word (tests/test_gpu_deep_bounded.py's list): 0 in these frames
FAILURES = ("long_safety_quits", "stranded_pixels", "check_dropped", "linger_expiries", "long_closed", "wide_overflows")
SPHERE_CAMERA = (-1.5, 0.7, -0.6, 0.785, 0.0, 0.7, 0.0)  # 0.75 from room_small's glass sphere (test_gpu_deep_bounded.py)


def _no_failures(dev):
    assert all(dev[k] == 0 for k in FAILURES), dev


@pytest.fixture(scope="module")
def room_small():
    """the scene on the device and the oracle's 96 x 64 frame of 2 passes (one call) — computed once"""
    run = helpers.GpuRun("room_small")
    ref, _ = helpers.oracle_render(run.path, 96, 64, 2)
    return run, ref


def test_cornell_equals_the_oracle():
    run = helpers.GpuRun("cornell")
    gpu, _, _ = run.render(64, 64, 4, **BOUNDED)
    ref, _ = helpers.oracle_render(run.path, 64, 64, 4)
    helpers.assert_bitwise(gpu, ref, what="cornell 64x64x4")


def test_duplicate_triangles_equal_the_oracle(tmp_path):
    dup = hazards.cornell_variant(str(tmp_path / "u"), "duplicate", yaw_room=0.1, extra_obj=hazards.DUPLICATE_OBJ)
    run = helpers.GpuRun(dup)
    gpu, _, _ = run.render(64, 64, 2, **BOUNDED)
    ref, _ = helpers.oracle_render(dup, 64, 64, 2)
    helpers.assert_bitwise(gpu, ref, what="duplicated quad 64x64x2")


def test_adversarial_near_equals_the_oracle(tmp_path):
    near = hazards.adversarial_scene(str(tmp_path / "near"), "near")
    run = helpers.GpuRun(near)
    gpu, _, _ = run.render(64, 64, 2, **BOUNDED)
    ref, _ = helpers.oracle_render(near, 64, 64, 2)
    helpers.assert_bitwise(gpu, ref, what="adversarial near 64x64x2")


def test_room_small_guard_on_every_ray(room_small):
    run, ref = room_small
    rt.deviation_stats(reset=True)
    gpu, _, _ = run.render(96, 64, 2, check_interval=1, **BOUNDED)
    dev = rt.deviation_stats(reset=True)
    helpers.assert_bitwise(gpu, ref, what="room_small 96x64x2, guard on every ray")
    assert dev["bounded_checked"] >= 96 * 64 * 2 and dev["bounded_mismatches"] == 0, dev
    _no_failures(dev)


def test_room_small_two_chained_calls(room_small):
    run, _ = room_small
    ref, _ = helpers.oracle_render(run.path, 96, 64, [1, 1])
    rt.deviation_stats(reset=True)
    gpu, _, _ = run.render(96, 64, [1, 1], overlap=True, coalesce_passes=-1, check_interval=1, **BOUNDED)
    dev = rt.deviation_stats(reset=True)
    helpers.assert_bitwise(gpu, ref, what="room_small 96x64, calls of 1 + 1 passes chained")
    assert dev["bounded_checked"] > 0 and dev["bounded_mismatches"] == 0, dev
    _no_failures(dev)


@pytest.fixture(scope="module")
def sphere():
    """room_small's sphere view, 96 x 64, 2 passes: the oracle's frames (one call; 1 + 1 calls), computed once,
    and the proof that the frame cannot pass without entering wf_long"""
    run = helpers.GpuRun("room_small")
    osc = oracle.OracleScene(run.path)
    cam = np.asarray(SPHERE_CAMERA, np.float32)
    dev = {}
    one, tot = helpers.oracle_render(run.path, 96, 64, 2, scene=osc, camera=cam, deviations=dev)
    two, _ = helpers.oracle_render(run.path, 96, 64, [1, 1], scene=osc, camera=cam)
    # the oracle's own paths go far past the hand-off depth: at least one ends 64 bounces deep or deeper
    deepest = max(64 * 2 ** k for k, h in enumerate(dev["deep_hist"]) if h)
    assert tot["maxdepth"] > 2 * LONG and deepest >= 4 * LONG, (tot, dev["deep_hist"])
    return run, cam, one, two, deepest


def _sphere_frame(run, cam_arr, passes, overlap):
    c = rt.Camera()
    c.position.x, c.position.y, c.position.z = (float(v) for v in cam_arr[:3])
    c.yaw, c.pitch, c.FOV, c.aperture_radius = (float(v) for v in cam_arr[3:7])
    g = rt.GBuffer(96, 64)
    for k, pc in enumerate(passes):
        rt.render(run.dev, g, c, 0 if k == 0 else 1,
                  rt.options(96, 64, pc, adaptive=False, wf_long_depth=LONG, coalesce_passes=-1, overlap=overlap,
                             check_interval=1, **BOUNDED))
    rt.join()
    return g.download()


@pytest.mark.parametrize("passes,overlap", [([2], False), ([1, 1], True)], ids=["one-call", "two-chained-calls"])
def test_sphere_view_shortest_long_depth(sphere, passes, overlap):
    """paths deeper than 16 bounces leave for wf_long, which returns the pixel or finishes it: the hand-off,
    wf_long's claim and release, the return ring; chained: the second call meets pixels still held"""
    run, cam, one, two, deepest = sphere
    rt.deviation_stats(reset=True)
    gpu = _sphere_frame(run, cam, passes, overlap)
    dev = rt.deviation_stats(reset=True)
    helpers.assert_bitwise(gpu, one if len(passes) == 1 else two, what=f"room_small sphere 96x64, calls {passes}, wf_long_depth 16")
    # the deep path ran here too (RtDeviations records paths that end 64 bounces deep or deeper), and with the ring
    # never closed (long_closed, below) a path past depth 16 is handed over: it ran in wf_long
    assert dev["deep_paths"] > 0 and dev["max_deep_depth"] >= deepest, dev
    assert dev["bounded_checked"] >= 96 * 64 * 2 and dev["bounded_mismatches"] == 0, dev
    _no_failures(dev)
    print("calls", passes, "deepest path", dev["max_deep_depth"], "owed pixels / passes", dev["owed_pixels"], dev["owed_passes"])
