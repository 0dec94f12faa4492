"""What rt_reproject buys and what it costs.

Error: an orbit of K cameras around the scene at S spp per frame (room_small
at 480x270, K = 16, S = 4 by default).  At every move the frame is either
reset (the reference's main()) or carried over by rt_reproject and S passes
added; the last frame's mean radiance is compared (mean squared error) with a
REF_SPP render of the last camera, before and after rt_denoise.  One JSON line
per configuration; --sweep runs the grid of max_history x depth_tol x
normal_min the defaults were chosen from.

Time: rt_reproject's device time on a 1920x1080 frame of the timing scene
(room2m by default) after a small camera move, by HIP events around batches
of BATCH calls on a stream, beside a device-to-device copy of the same three
arrays (frame_buffer, squared_luminance, sample_count) timed the same way in
the same loop — the floor of any pass that must write them.

usage: python tools/reproject_bench.py [--scene NAME] [--size W H] [--frames K] [--spp S] [--sweep]
                                       [--time-scene NAME | --no-time] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

import gpu_timing

import helpers  # noqa: E402
import rt  # noqa: E402

REF_SPP = 2048
WARMUP, REPS, BATCH = 3, 20, 50
ORBIT_STEP, ORBIT_RADIUS = -0.02, 2.4  # radians per frame about the point this far in front of the scene's camera
GRID = [dict(max_history=m, depth_tol=d, normal_min=c) for m in (16, 32, 64, 128) for d in (0.01, 0.02, 0.05)
        for c in (0.8, 0.9, 0.95)]
# the same tolerances where no triangle buffer decides first (equal ids imply a close depth and normal)
GRID += [dict(match_triangle=False, depth_tol=d, normal_min=c) for d in (0.01, 0.02, 0.05) for c in (0.8, 0.9, 0.95)]


def orbit(cam, angle, radius=ORBIT_RADIUS):
    yaw = cam.yaw + angle
    cx, cz = cam.position.x + radius * np.sin(cam.yaw), cam.position.z + radius * np.cos(cam.yaw)
    return rt.Camera(rt.Vec3D(cx - radius * np.sin(yaw), cam.position.y, cz - radius * np.cos(yaw)), yaw, cam.pitch,
                     cam.FOV, cam.aperture_radius)


def mse(mean, truth, valid):
    """over the pixels whose reference is finite (the renderer, like the reference, can return a NaN sample)"""
    return float(np.mean((mean.astype(np.float64).reshape(-1, 3)[valid] - truth[valid]) ** 2))


def frame_mean(g):
    fb, _, cnt, _ = g.download()
    return fb / np.maximum(cnt, 1)[:, None].astype(np.float32), cnt


def error_lines(scene, W, H, K, S, configs):
    run = helpers.GpuRun(scene)
    cams = [orbit(run.camera, ORBIT_STEP * k) for k in range(K)]
    aovs = [rt.render_aov(run.dev, c, W, H) for c in cams]
    opt = rt.options(W, H, S, adaptive=False, kernel=rt.KERNEL_WAVEFRONT)
    g = rt.GBuffer(W, H)
    for c in range(REF_SPP // 256):
        rt.render(run.dev, g, cams[-1], 0 if c == 0 else 1,
                  rt.options(W, H, 256, adaptive=False, kernel=rt.KERNEL_WAVEFRONT))
    rt.join()
    truth, cnt = frame_mean(g)
    assert (cnt == REF_SPP).all()
    truth = truth.astype(np.float64)
    valid = np.isfinite(truth).all(axis=1)
    hits = float(np.isfinite(aovs[-1]["depth"]).mean())
    rt.render(run.dev, g, cams[-1], 0, opt)  # "reset every frame": the last frame is S fresh samples
    rt.join()
    reset = {"raw": mse(frame_mean(g)[0], truth, valid), "denoised": mse(rt.denoise(g, aovs[-1]), truth, valid)}
    g.free()
    lines = []
    for cfg in configs:
        g = rt.GBuffer(W, H)
        rt.render(run.dev, g, cams[0], 0, opt)
        kept = []
        for k in range(1, K):
            g_k, st = rt.reproject(g, aovs[k - 1], cams[k - 1], aovs[k], cams[k], stats=True, **cfg)
            g.free()
            g = g_k
            kept.append(st["kept_pixels"] / (W * H))
            rt.render(run.dev, g, cams[k], 1, opt)
        rt.join()
        mean, cnt = frame_mean(g)
        e_raw, e_den = mse(mean, truth, valid), mse(rt.denoise(g, aovs[-1]), truth, valid)
        g.free()
        lines.append({"scene": scene, "width": W, "height": H, "frames": K, "spp_per_frame": S, "ref_spp": REF_SPP,
                      "options": cfg or "defaults", "mse_reset": reset["raw"], "mse_reset_denoised": reset["denoised"],
                      "mse_reprojected": e_raw, "mse_reprojected_denoised": e_den,
                      "ratio": e_raw / reset["raw"], "ratio_denoised": e_den / reset["denoised"],
                      "history_kept_mean": float(np.mean(kept)), "history_kept_min": float(min(kept)),
                      "hit_pixels_last_frame": hits, "reference_pixels_not_finite": int((~valid).sum()),
                      "mean_count_last_frame": float(cnt.mean())})
    return lines


def spread(ms):
    s = gpu_timing.summary(ms, 5)
    return {"median_ms": s["ms_median"], "min_ms": s["ms_min"], "max_ms": s["ms_max"], "reps": s["reps"]}


def timing_line(scene, W=1920, H=1080):
    hip = gpu_timing.hip()
    L = rt.lib()
    n = W * H
    run = helpers.GpuRun(scene)
    cam_a = run.camera
    cam_b = orbit(cam_a, ORBIT_STEP)
    g, out = rt.GBuffer(W, H), rt.GBuffer(W, H)
    rt.render(run.dev, g, cam_a, 0, rt.options(W, H, 4, adaptive=False, kernel=rt.KERNEL_WAVEFRONT))
    rt.join()
    bufs = []

    def guides(cam):
        ptrs = [rt.DeviceArray(n, np.float32), rt.DeviceArray((n, 3), np.float32), rt.DeviceArray(n, np.int32)]
        bufs.extend(ptrs)
        b = rt.RtAovBuffers(ptrs[0].p, ptrs[1].p, None, ptrs[2].p)
        rt.check(L.rt_render_aov(run.dev.prepared, cam, W, H, ctypes.byref(b), None))
        return ptrs
    ga, gb = guides(cam_a), guides(cam_b)
    d_stats = rt.DeviceArray(3, np.uint64, zero=True)
    bufs.append(d_stats)
    rt.reproject_device(g.g, ga, cam_a, gb, cam_b, W, H, out.g, stats=d_stats)
    st = d_stats.read()
    timer = gpu_timing.Timer()
    s = timer.stream
    arrays = [(out.g.frame_buffer, g.g.frame_buffer, n * 12), (out.g.squared_luminance, g.g.squared_luminance, n * 4),
              (out.g.sample_count, g.g.sample_count, n * 4)]

    # A batch is enqueued behind a render pass of the frame on the same stream, so the device still has work
    # when the host has finished enqueueing: the events then span the batch's device time, not the host's
    # enqueue rate (host_ms is that rate: the measurement holds while it is below the render's time)
    busy = rt.GBuffer(W, H)
    busy_opt = rt.options(W, H, 2, adaptive=False, kernel=rt.KERNEL_WAVEFRONT, stream=s.value)
    host_ms = {}

    def timed(work, name):
        rt.render(run.dev, busy, cam_a, 0, busy_opt)
        t = time.perf_counter()
        timer.start()
        for _ in range(BATCH):
            work()
        timer.stop()
        host_ms.setdefault(name, []).append((time.perf_counter() - t) * 1e3)
        timer.synchronize()
        host_ms.setdefault(name + "_with_wait", []).append((time.perf_counter() - t) * 1e3)
        return timer.elapsed_ms() / BATCH

    def do_reproject():
        rt.reproject_device(g.g, ga, cam_a, gb, cam_b, W, H, out.g, stream=s.value)

    def do_copy():
        for dst, src, nbytes in arrays:
            assert hip.hipMemcpyAsync(dst, src, nbytes, 3, s) == 0  # hipMemcpyDeviceToDevice
    t_rp, t_cp = [], []
    for r in range(WARMUP + REPS):  # alternating, in one loop: the two see the same machine
        a, b = timed(do_reproject, "reproject"), timed(do_copy, "copy")
        if r >= WARMUP:
            t_rp.append(a)
            t_cp.append(b)
    timer.close()
    for d in bufs:
        d.free()
    g.free()
    out.free()
    busy.free()
    rp, cp = spread(t_rp), spread(t_cp)
    # unique bytes per pixel: dst depth, normal, triangle in (20); src count, depth, normal, triangle, fb, sq in
    # (36, each source pixel read once under coherent motion); fb, sq, count out (20)
    return {"timing_scene": scene, "width": W, "height": H, "batch": BATCH, "reproject": rp, "copy_fb_sq_count": cp,
            "reproject_over_copy": round(rp["median_ms"] / cp["median_ms"], 3),
            "unique_mb": round(n * 76 / 1e6, 1), "reproject_gb_s": round(n * 76 / rp["median_ms"] / 1e6, 1),
            "copy_gb_s": round(n * 40 / cp["median_ms"] / 1e6, 1), "history_kept": float(st[1]) / n,
            "host_enqueue_ms_per_batch": {k: gpu_timing.summary(v, 3)["ms_median"] for k, v in host_ms.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="room_small")
    ap.add_argument("--size", nargs=2, type=int, default=[480, 270])
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--time-scene", default="room2m")
    ap.add_argument("--no-time", action="store_true")
    ap.add_argument("--no-error", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    gpu_timing.require_device("reproject_bench")
    lines = []
    if not a.no_error:
        lines += error_lines(a.scene, a.size[0], a.size[1], a.frames, a.spp, [{}] + (GRID if a.sweep else []))
    if not a.no_time:
        lines.append(timing_line(a.time_scene))
    text = "".join(json.dumps(line) + "\n" for line in lines)
    sys.stdout.write(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
