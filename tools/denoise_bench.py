"""Time of rt_denoise on a 1920x1080 frame, beside two yardsticks: the
compulsory HBM traffic of its passes at the achievable HBM rate, and one
1-spp rt_render pass of the same frame measured in the same run (does
denoising cost more or less than one more pass?).

The frame is a 4-spp render of the scene (room_small by default; room2m is
the bench scene), its guides rt_render_aov's.  rt_denoise is enqueued on a
stream in batches of BATCH calls ended by a stream synchronise (a launch
returns before its kernels finish); the time per call of REPS batches gives
the median and the spread.  Timed at 1 to 5 levels (5 is the default): the
increments are the levels' own times — tap spacing 1 and 2, where a tile's
taps overlap in the CU's vector cache, against 4, 8 and 16, where they do
not — and the 1-level time less a level's is the prepare pass's.

usage: python tools/denoise_bench.py [scene] [width height] [--out FILE]
Prints one JSON object (also written to FILE).
"""
import ctypes
import json
import os
import sys
import time

import numpy as np

import gpu_timing

import helpers  # noqa: E402
import rt  # noqa: E402

WARMUP, REPS, BATCH = 3, 20, 5
HBM_TBS = 6.3  # achievable HBM bandwidth of the MI355X, TB/s (8 peak)

# compulsory bytes per pixel: what each pass must read and write once
PREPARE_B = (12 + 4 + 4) + (4 + 12 + 12) + (16 + 16 + 4)  # G_Buffer + AOVs in, state + guides + slope out
LEVEL_B = (16 + 16) + (16 + 4)                            # state in and out, guides + slope
LAST_LEVEL_B = 16 + (16 + 4) + 12 + 12                    # state in, guides, albedo in, RGB out


def traffic_bytes(pixels, iterations):
    return pixels * (PREPARE_B + (iterations - 1) * LEVEL_B + LAST_LEVEL_B)


def spread(ms):
    s = gpu_timing.summary(ms, 4)
    return {"median_ms": s["ms_median"], "min_ms": s["ms_min"], "max_ms": s["ms_max"], "reps": s["reps"]}


def main():
    args = [a for a in sys.argv[1:]]
    out_file = None
    if "--out" in args:
        i = args.index("--out")
        out_file = args[i + 1]
        del args[i:i + 2]
    scene = args[0] if args else "room_small"
    W, H = (int(args[1]), int(args[2])) if len(args) >= 3 else (1920, 1080)
    n = W * H
    gpu_timing.require_device("denoise_bench")
    L = rt.lib()
    run = helpers.GpuRun(scene)
    g = rt.GBuffer(W, H)
    rt.render(run.dev, g, run.camera, 0, rt.options(W, H, 4, adaptive=False, kernel=rt.KERNEL_WAVEFRONT))
    rt.join()
    f32 = np.float32
    d_depth, d_normal, d_albedo = rt.DeviceArray(n, f32), rt.DeviceArray((n, 3), f32), rt.DeviceArray((n, 3), f32)
    d_out = rt.DeviceArray((n, 3), f32)
    b = rt.RtAovBuffers(d_depth.p, d_normal.p, d_albedo.p, None)
    rt.check(L.rt_render_aov(run.dev.prepared, run.camera, W, H, ctypes.byref(b), None))
    timer = gpu_timing.Timer()

    result = {"scene": scene, "width": W, "height": H, "batch": BATCH, "hbm_tb_s": HBM_TBS, "denoise": {}}
    for iterations in (1, 2, 3, 4, 5):
        ms = []
        for r in range(WARMUP + REPS):  # (a host-clock batch: a launch returns before its kernels finish)
            timer.synchronize()
            t = time.perf_counter()
            for _ in range(BATCH):
                rt.denoise_device(g.g, (d_depth, d_normal, d_albedo), W, H, d_out, iterations=iterations,
                                  stream=timer.s)
            timer.synchronize()
            if r >= WARMUP:
                ms.append((time.perf_counter() - t) * 1e3 / BATCH)
        e = spread(ms)
        e["compulsory_mb"] = round(traffic_bytes(n, iterations) / 1e6, 1)
        e["hbm_floor_ms"] = round(traffic_bytes(n, iterations) / (HBM_TBS * 1e12) * 1e3, 4)
        e["times_hbm_floor"] = round(e["median_ms"] / e["hbm_floor_ms"], 2)
        result["denoise"][f"iterations_{iterations}"] = e
    d5, d1 = result["denoise"]["iterations_5"]["median_ms"], result["denoise"]["iterations_1"]["median_ms"]
    med = [result["denoise"][f"iterations_{k}"]["median_ms"] for k in (1, 2, 3, 4, 5)]
    # level k's own time (spacing 2^k), k = 1..4: what one more level costs
    result["level_ms_by_spacing"] = {str(1 << k): round(med[k] - med[k - 1], 4) for k in (1, 2, 3, 4)}
    result["per_level_ms"] = round((d5 - d1) / 4, 4)
    result["prepare_ms"] = round(d1 - (d5 - d1) / 4, 4)

    # one more 1-spp pass of the same frame (synchronous calls: each ends in a device synchronise)
    ms = []
    opt = rt.options(W, H, 1, adaptive=False, kernel=rt.KERNEL_WAVEFRONT)
    for r in range(WARMUP + REPS):
        t = time.perf_counter()
        rt.render(run.dev, g, run.camera, 1, opt)
        rt.check(L.rt_synchronize())
        if r >= WARMUP:
            ms.append((time.perf_counter() - t) * 1e3)
    result["render_1spp"] = spread(ms)
    result["denoise_over_render_1spp"] = round(d5 / result["render_1spp"]["median_ms"], 3)

    timer.close()
    for d in (d_depth, d_normal, d_albedo, d_out):
        d.free()
    g.free()
    line = json.dumps(result)
    print(line)
    if out_file:
        os.makedirs(os.path.dirname(os.path.abspath(out_file)), exist_ok=True)
        with open(out_file, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
