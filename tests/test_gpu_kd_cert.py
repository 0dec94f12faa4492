"""GPU checks of the T* certificate (csrc/bvh_trace.h kd_certified, DESIGN.md §5
"The certificate").  The bounded traversal is the default, so every other GPU
test already runs the certificate; this file adds what they lack:

* the run-time guard on EVERY ray (check_interval=1: each finisher ray is
  re-traced by the plain KD traversal and compared bit for bit) on Cornell,
  the hazard scenes and the adversarial "near" frame;
* counted calls: the certificate is really taken on Cornell, and really
  refused where every hit is a tie (the duplicated quad), whose frame —
  the deferred-descent scheduler under load — equals the KD traversal's;
* the glass light guide with deep paths in wf_long (the certificate on the
  wave's one ray, and the hand-off), chained calls against one call.

The counted tests read the certificate's two counters (rt_kd_cert_stats:
certified and fallback hit rays of the counting instantiations).
"""
import numpy as np
import pytest

import hazards
import helpers
import oracle
import rt

pytestmark = pytest.mark.gpu
WF = rt.KERNEL_WAVEFRONT


def _guarded(run, W, H, passes, cam_arr=None, rng0=None):
    """a bounded render with the guard on every ray; returns the deviation block"""
    n = W * H
    g = rt.GBuffer(W, H)
    if rng0 is not None:
        g.upload(np.zeros((n, 3), np.float32), np.zeros(n, np.float32), np.zeros(n, np.int32), rng0)
    cam = run.camera
    if cam_arr is not None:
        cam = rt.Camera()
        cam.position.x, cam.position.y, cam.position.z = (float(v) for v in cam_arr[:3])
        cam.yaw, cam.pitch, cam.FOV, cam.aperture_radius = (float(v) for v in cam_arr[3:7])
    rt.deviation_stats(reset=True)
    for c, p in enumerate(passes):
        rt.render(run.dev, g, cam, 0 if c == 0 else 1,
                  rt.options(W, H, p, adaptive=False, kernel=WF, traversal=rt.TRAVERSAL_BOUNDED, check_interval=1))
    rt.join()
    dev = rt.deviation_stats(reset=True)
    assert dev["bounded_checked"] > 0 and dev["bounded_mismatches"] == 0 and dev["check_dropped"] == 0, dev
    return dev


def test_guard_on_every_ray_cornell():
    dev = _guarded(helpers.GpuRun("cornell"), 64, 64, [4])
    assert dev["bounded_checked"] >= 64 * 64 * 4, dev  # at least the camera rays


def test_guard_on_every_ray_hazard_scenes(tmp_path):
    W, H, P = 40, 32, 3
    seeds = oracle.mt19937(W * H)
    _guarded(helpers.GpuRun(hazards.cornell_variant(str(tmp_path / "a"), "aligned", yaw_room=0.0)), W, H, [P], rng0=seeds)
    cornell = helpers.scene_path("cornell")
    on, _ = hazards.h5_cameras(oracle.OracleScene(cornell))
    _guarded(helpers.GpuRun(cornell), W, H, [P], cam_arr=on, rng0=seeds)
    axis = hazards.cornell_variant(str(tmp_path / "x"), "aligned", yaw_room=0.0, camera=hazards.AXIS_CAMERA)
    _guarded(helpers.GpuRun(axis), W, H, [P], rng0=hazards.h7_axis_seeds(W, H))
    degen = hazards.cornell_variant(str(tmp_path / "d"), "degenerate", yaw_room=0.1, extra_obj=hazards.DEGENERATE_OBJ)
    _guarded(helpers.GpuRun(degen), W, H, [P], rng0=seeds)
    dup = hazards.cornell_variant(str(tmp_path / "u"), "duplicate", yaw_room=0.1, extra_obj=hazards.DUPLICATE_OBJ)
    _guarded(helpers.GpuRun(dup), W, H, [P], rng0=seeds)
    _guarded(helpers.GpuRun(helpers.make_trap_scene(str(tmp_path / "t"))), W, H, [P], rng0=seeds)


def test_guard_on_every_ray_adversarial_near(tmp_path):
    run = helpers.GpuRun(hazards.adversarial_scene(str(tmp_path / "near"), "near"))
    dev = _guarded(run, 320, 240, [4, 4])
    assert dev["bounded_checked"] >= 320 * 240 * 8, dev


def test_counted_call_takes_the_certificate_on_cornell():
    """certified + fallback = the hit rays (fallback: found by a KD descent)"""
    run = helpers.GpuRun("cornell")
    rt.kd_cert_stats(reset=True)
    _, cnt, _ = run.render(64, 64, 4, count=True, kernel=WF, traversal=rt.TRAVERSAL_BOUNDED_COUNTED)
    certified, fallback = rt.kd_cert_stats(reset=True)
    print("cornell 64x64x4: certified", certified, "fallback", fallback, "hits", cnt["hit"], "KD nodes", cnt["node"])
    assert certified > 0, (certified, fallback, cnt)
    assert certified + fallback == cnt["hit"], (certified, fallback, cnt)
    _, kcnt, _ = run.render(64, 64, 4, count=True, kernel=WF)  # the counting build: the KD traversal
    assert cnt["hit"] == kcnt["hit"] and cnt["ray"] == kcnt["ray"], (cnt, kcnt)


def test_counted_call_falls_back_on_duplicate_triangles(tmp_path):
    """Every hit on the duplicated quad is a tie: no certificate, the descent runs (deferred, many lanes
    of a wave at once) — and the frame is the KD traversal's.  Against the same room without the quad
    (same camera, same seeds) the hits found by a descent grow and the certified share drops."""
    W, H, P = 64, 64, 4

    def counted(path):
        run = helpers.GpuRun(path)
        rt.kd_cert_stats(reset=True)
        _, cnt, _ = run.render(W, H, P, count=True, kernel=WF, traversal=rt.TRAVERSAL_BOUNDED_COUNTED)
        certified, fallback = rt.kd_cert_stats(reset=True)
        assert certified + fallback == cnt["hit"] and cnt["hit"] > W * H, (certified, fallback, cnt)
        return run, certified, fallback

    _, c0, f0 = counted(hazards.cornell_variant(str(tmp_path / "p"), "plain", yaw_room=0.1))
    dup = hazards.cornell_variant(str(tmp_path / "u"), "duplicate", yaw_room=0.1, extra_obj=hazards.DUPLICATE_OBJ)
    run, c1, f1 = counted(dup)
    print("64x64x4 certified / fallback: plain room", c0, f0, "with the duplicated quad", c1, f1)
    # Hits on the quad are ties: never certified, where the same rays' hits on the walls behind it were certified
    # at the room's rate.  (No count of them is asserted: paths differ after their first hit on the quad, so the two
    # frames' totals are not the quad's hits apart.  Measured: 31,550 / 10,212 plain, 30,669 / 10,986 with the quad.)
    assert f1 > f0 and c1 < c0, (c0, f0, c1, f1)
    assert c1 * (c0 + f0) < c0 * (c1 + f1), (c0, f0, c1, f1)  # certified share: lower with the quad
    a, _, _ = run.render(W, H, P, kernel=WF, traversal=rt.TRAVERSAL_BOUNDED)
    b, _, _ = run.render(W, H, P, kernel=WF, traversal=rt.TRAVERSAL_KD)
    helpers.assert_bitwise(a, b, what="duplicate quad: bounded vs kd")


def test_light_guide_deep_paths_chained_vs_one_call(tmp_path):
    run = helpers.GpuRun(helpers.make_trap_scene(str(tmp_path / "t")))
    W, H, split = 48, 32, [1, 1, 2]
    rt.deviation_stats(reset=True)
    one, _, _ = run.render(W, H, [sum(split)], kernel=WF, overlap=False, wf_long_depth=16, coalesce_passes=-1)
    chained, _, _ = run.render(W, H, split, kernel=WF, overlap=True, wf_long_depth=16, coalesce_passes=-1)
    dev = rt.deviation_stats(reset=True)
    helpers.assert_bitwise(chained, one, what="light guide: chained calls vs one call")
    assert dev["deep_paths"] > 0, dev  # paths really went through wf_long
    assert dev["stranded_pixels"] == 0 and dev["long_safety_quits"] == 0, dev
