"""wf_long's bounded deep bounces (csrc/wide_bvh.h: the wave-wide,
level-synchronous s_min query over the wide collapse of the conservative BVH,
then the bounded KD traversal run by the same wave) against the oracle, bit for bit
(fb, sq, count, RNG state), at the whole-call hand-off's minimum depth
(wf_long_depth 16) so that the frames' deep paths run in wf_long:

* the glass light guide (every path deep);
* a small frame of room_small aimed at a glass sphere, whose oracle render
  shows (asserted from its depth histogram) more than 1,000 bounces past the
  hand-off depth — unchained, and as two chained calls followed by a join;
* the hazard scenes (walls on split planes, axis-parallel camera rays, the
  camera on the root split) and an axis-aligned glass block in the aligned
  room, whose deep bounces start on split planes (the non-bounded fallback);
* the run-time guard on the room_small frame with every hand-off failure
  counter and the overflow word at 0.  The guard samples the FINISHER's rays
  only (here: every one of them re-traced); wf_long's bounces are not
  recorded for it, so what checks them is the comparison with the oracle;
* the forced overflow (RT_DEBUG_WIDE_CAP1): every query abandoned and the ray
  traced by the wide KD traversal — identical frame, overflow word > 0.

The host restatement of the query is checked in tests/test_wide_smin_host.py.
"""
import numpy as np
import pytest

import hazards
import helpers
import oracle
import rt

pytestmark = pytest.mark.gpu
WF = rt.KERNEL_WAVEFRONT
LONG = 16  # the hand-off's minimum depth (wavefront.hip WF_LONG_DEPTH_MIN)
FAILURES = ("long_safety_quits", "stranded_pixels", "check_dropped", "linger_expiries", "long_closed")


def _camera(arr):
    c = rt.Camera()
    c.position.x, c.position.y, c.position.z = float(arr[0]), float(arr[1]), float(arr[2])
    c.yaw, c.pitch, c.FOV, c.aperture_radius = float(arr[3]), float(arr[4]), float(arr[5]), float(arr[6])
    return c


def _gpu(run, W, H, passes, cam_arr, rng0=None, **kw):
    """`passes`: the passes of each call (chained when overlap=True), then a join"""
    n = W * H
    g = rt.GBuffer(W, H)
    if rng0 is not None:
        g.upload(np.zeros((n, 3), np.float32), np.zeros(n, np.float32), np.zeros(n, np.int32), rng0)
    cam = _camera(cam_arr)
    for c, pc in enumerate(passes):
        rt.render(run.dev, g, cam, 0 if c == 0 else 1,
                  rt.options(W, H, pc, adaptive=False, kernel=WF, wf_long_depth=LONG, coalesce_passes=-1, **kw))
    rt.join()
    return g.download()


def _bounces_past(hist, depth):
    """a lower bound, from the oracle's histogram of paths that ended at depth >= 64 (bin k:
    [64 * 2^k, 64 * 2^(k+1))), of the bounces its paths made past `depth`"""
    return sum(int(h) * (64 * 2 ** k - depth) for k, h in enumerate(hist))


# ------------------------------------------------------------ the light guide
def test_light_guide_every_path_deep(tmp_path):
    trap = helpers.make_trap_scene(str(tmp_path / "t"), length=12.0)
    run = helpers.GpuRun(trap)
    osc = oracle.OracleScene(trap)
    W, H, P = 16, 2, 2
    ref, tot = helpers.oracle_render(trap, W, H, P, scene=osc)
    assert tot["maxdepth"] > 2 * LONG, tot  # the paths do go past the hand-off depth
    rt.deviation_stats(reset=True)
    gpu = _gpu(run, W, H, [P], osc.camera)
    helpers.assert_bitwise(gpu, ref, what="light guide, deep paths in wf_long")
    dev = rt.deviation_stats(reset=True)
    assert dev["wide_overflows"] == 0 and all(dev[k] == 0 for k in FAILURES), dev


# ------------------------------------------------------------ room_small, a glass sphere
# A camera 0.75 from the glass sphere at (-1.0, 0.45, -0.1), found on the CPU: over these 8 passes
# the oracle shows a path of more than 10^4 bounces inside the sphere (total internal reflection)
ROOM_W, ROOM_H, ROOM_P = 48, 27, 8
ROOM_CAMERA = (-1.5, 0.7, -0.6, 0.785, 0.0, 0.7, 0.0)


@pytest.fixture(scope="module")
def room():
    run = helpers.GpuRun("room_small")
    osc = oracle.OracleScene(run.path)
    cam = np.asarray(ROOM_CAMERA, np.float32)
    dev = {}
    ref, tot = helpers.oracle_render(run.path, ROOM_W, ROOM_H, ROOM_P, scene=osc, camera=cam, deviations=dev)
    # the frame cannot pass by never entering wf_long: the oracle's own paths go far past the hand-off depth
    assert _bounces_past(dev["deep_hist"], LONG) >= 1000, (dev["deep_hist"], tot)
    return run, cam, ref


@pytest.mark.parametrize("split,overlap", [([ROOM_P], False), ([ROOM_P // 2, ROOM_P // 2], True)],
                         ids=["unchained", "two-chained-calls"])
def test_room_small_sphere(room, split, overlap):
    run, cam, ref = room
    rt.deviation_stats(reset=True)
    gpu = _gpu(run, ROOM_W, ROOM_H, split, cam, overlap=overlap)
    helpers.assert_bitwise(gpu, ref, what=f"room_small sphere, calls {split}")
    dev = rt.deviation_stats(reset=True)
    assert dev["max_deep_depth"] > 1000, dev  # the deep path ran here too
    assert dev["wide_overflows"] == 0 and all(dev[k] == 0 for k in FAILURES), dev


def test_room_small_sphere_guard(room):
    """check_interval = 1: every ray of the finisher re-traced by the plain KD traversal.  (wf_long's
    own bounces are not sampled by the guard: bounded_checked / bounded_mismatches say nothing about
    them — the bitwise comparison with the oracle does.)"""
    run, cam, ref = room
    rt.deviation_stats(reset=True)
    gpu = _gpu(run, ROOM_W, ROOM_H, [ROOM_P], cam, check_interval=1)
    helpers.assert_bitwise(gpu, ref, what="room_small sphere, guard on every ray")
    dev = rt.deviation_stats(reset=True)
    assert dev["bounded_checked"] > 0 and dev["bounded_mismatches"] == 0, dev
    assert dev["wide_overflows"] == 0 and all(dev[k] == 0 for k in FAILURES), dev


def test_room_small_sphere_forced_overflow(room):
    """RT_DEBUG_WIDE_CAP1: the query's lists hold one item, so every query that meets two children
    is abandoned and its ray traced by the wide KD traversal — the same frame"""
    run, cam, ref = room
    rt.deviation_stats(reset=True)
    gpu = _gpu(run, ROOM_W, ROOM_H, [ROOM_P], cam, debug=rt.DEBUG_WIDE_CAP1)
    helpers.assert_bitwise(gpu, ref, what="room_small sphere, every query overflowing")
    dev = rt.deviation_stats(reset=True)
    assert dev["wide_overflows"] > 1000, dev
    assert all(dev[k] == 0 for k in FAILURES), dev


# ------------------------------------------------------------ hazard scenes
GLASS_MAT = "\nmaterial hzglass\nalbedo 0.995 0.995 0.995\nroughness 0.001\nn 1.51\ntransparent\n"


def _block(x0, x1, y0, y1, z0, z1):
    """an axis-aligned glass block (appended to cornell.obj: relative vertex indices)"""
    v = [(x0, y0, z0), (x1, y0, z0), (x1, y1, z0), (x0, y1, z0), (x0, y0, z1), (x1, y0, z1), (x1, y1, z1), (x0, y1, z1)]
    s = "\nusemtl hzglass\n" + "".join(f"v {a} {b} {c}\n" for a, b, c in v)
    for f in ("-8 -5 -6 -7", "-4 -3 -2 -1", "-8 -7 -3 -4", "-5 -1 -2 -6", "-8 -4 -1 -5", "-7 -6 -2 -3"):
        s += "f " + f + "\n"
    return s


def _hazard_case(name, d):
    """(scene path, camera or None for the scene's, seeds or None, passes)"""
    if name == "walls-on-splits":
        return hazards.cornell_variant(d, "aligned", yaw_room=0.0), None, None, 8
    if name == "axis-parallel-rays":
        p = hazards.cornell_variant(d, "aligned", yaw_room=0.0, camera=hazards.AXIS_CAMERA)
        return p, None, hazards.h7_axis_seeds(40, 32), 8
    if name == "camera-on-root-split":
        p = helpers.scene_path("cornell")
        return p, hazards.h5_cameras(oracle.OracleScene(p))[0], None, 8
    if name == "duplicate-triangles":
        return hazards.cornell_variant(d, "duplicate", yaw_room=0.1, extra_obj=hazards.DUPLICATE_OBJ), None, None, 8
    assert name == "glass-block-on-splits"
    p = hazards.cornell_variant(d, "glassblock", yaw_room=0.0, camera=hazards.AXIS_CAMERA,
                                extra_obj=_block(-0.4, 0.3, -0.5, 0.4, -0.3, 0.4), extra_mat=GLASS_MAT)
    return p, None, None, 4


@pytest.mark.parametrize("name", ["walls-on-splits", "axis-parallel-rays", "camera-on-root-split",
                                  "duplicate-triangles", "glass-block-on-splits"])
def test_hazard_scenes_at_handoff_depth(name, tmp_path):
    path, cam, rng0, P = _hazard_case(name, str(tmp_path / "h"))
    run = helpers.GpuRun(path)
    osc = oracle.OracleScene(path)
    cam = osc.camera if cam is None else cam
    W, H = 40, 32
    n = W * H
    rng0 = oracle.mt19937(n) if rng0 is None else rng0
    fb, sq, ct, rng = np.zeros(n * 3, np.float32), np.zeros(n, np.float32), np.zeros(n, np.int32), rng0.copy()
    k = osc.render(np.asarray(cam, np.float32), fb, sq, ct, rng, W, H, P, sample_count_arg=0, adaptive=False)
    if name == "glass-block-on-splits":  # deep bounces inside the block: wf_long is entered
        assert k["maxdepth"] > 2 * LONG and k["hazards"]["on_split"] > 1000, k
    rt.deviation_stats(reset=True)
    gpu = _gpu(run, W, H, [P], cam, rng0=rng0)
    helpers.assert_bitwise(gpu, (fb.reshape(n, 3), sq, ct, rng), what=name)
    dev = rt.deviation_stats(reset=True)
    assert dev["wide_overflows"] == 0 and all(dev[k2] == 0 for k2 in FAILURES), dev
