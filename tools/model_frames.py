"""A frame's whole life under any camera model (rt_sample_paths, rt_sample_aov,
rt_denoise_sampler, rt_reproject_sampler), and the timings of the three
sampler-frame calls beside what they replace.

The flow (default): on a generated scene, for one model —

    rt_sample_paths        --spp samples per pixel at camera A into a G_Buffer
    rt_sample_aov          the guides of camera A
    rt_denoise_sampler     a.png (the noisy frame) and a.denoised.png
    the camera moves       (--move dx dz dyaw)
    rt_sample_aov          the guides of camera B
    rt_reproject_sampler   the history carried to camera B: b.carried.png
    rt_sample_paths        --spp2 more samples on the carried G_Buffer
    rt_denoise_sampler     b.png and b.denoised.png

and one JSON line with the kept fraction and the sample counts.

--bench: on room2m, a 1920 x 960 equirectangular and a 1920 x 1080 fisheye
frame (and pinhole and orthographic ones for the reprojection), every call
between two device events on one stream, the variants alternating for --reps
rounds after a warm-up, as tools/sampler_bench.py does:

    sample_aov    rt_sample_aov against rt_sampler_rays(rng = NULL) + rt_trace_rays with a surface output
                  (checked bit for bit before the timing)
    denoise       rt_denoise_sampler against rt_denoise at the same size
    reproject     rt_reproject_sampler per kind against rt_reproject at the same size

One JSON line per variant (median, min, max of the event timings) in --out.

usage: python tools/model_frames.py [--model equirect] [--scene room_small] [--width 512 --height 256]
                                    [--spp 4 --spp2 4] [--move 0.04 0.03 0.02] [--out-dir DIR]
       python tools/model_frames.py --bench [--scene room2m] [--reps 10] [--warmup 2] [--out FILE]
"""
import argparse
import collections
import ctypes
import json
import os

import numpy as np

import gpu_timing
from gpu_timing import ROOT

import helpers  # noqa: E402
import rt  # noqa: E402

f32 = np.float32
AOV = ("depth", "normal", "albedo", "triangle")
# a timed variant: its comparison group, what sets its frame up (outside the span), the timed call, record fields
Variant = collections.namedtuple("Variant", "group prepare fn fields")


def model_sampler(run, kind, W, H, move=(0.0, 0.0, 0.0)):
    """the scene's camera under `kind` (fisheye: 3 rad across the image circle), moved by (dx, dz, dyaw)"""
    cam = run.camera
    cam = rt.Camera(rt.Vec3D(cam.position.x + move[0], cam.position.y, cam.position.z + move[1]), cam.yaw + move[2],
                    cam.pitch, 3.0 if kind == "fisheye" else cam.FOV, 0.0)
    return rt.Sampler(kind, W, H, cam, ortho_half_width=1.5)


def sample(run, smp, g, spp, accumulate):
    rt.sample_paths_device(run.dev, smp, g.g.random_numbers, smp.n, g.g.frame_buffer, g.g.squared_luminance,
                           g.g.sample_count, samples=spp, accumulate=accumulate)


def write_rgb(path, rgb):
    """an (H, W, 3) mean-radiance image (row 0 = bottom) as a PNG"""
    H, W = rgb.shape[:2]
    rgba = np.ascontiguousarray(rt.tonemap_rgb(rgb).reshape(H, W, 4)[::-1])
    L = rt.lib()
    L.rt_write_png.argtypes = [ctypes.c_char_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    rt.check(L.rt_write_png(path.encode(), rgba.ctypes.data, W, H))


def flow(a):
    W, H = a.width, a.height
    run = helpers.GpuRun(a.scene)
    os.makedirs(a.out_dir, exist_ok=True)
    out = lambda name: os.path.join(a.out_dir, f"{a.model}.{name}")  # noqa: E731
    smp_a, smp_b = model_sampler(run, a.model, W, H), model_sampler(run, a.model, W, H, a.move)
    g = rt.GBuffer(W, H)
    sample(run, smp_a, g, a.spp, False)
    aov_a = rt.sample_aov(run.dev, smp_a)
    rt.save_render(g, out("a.png"))
    write_rgb(out("a.denoised.png"), rt.denoise_sampler(g, aov_a, smp_a))
    aov_b = rt.sample_aov(run.dev, smp_b)
    carried, stats = rt.reproject_sampler(g, aov_a, smp_a, aov_b, smp_b, stats=True)
    g.free()
    rt.save_render(carried, out("b.carried.png"))
    sample(run, smp_b, carried, a.spp2, True)
    rt.save_render(carried, out("b.png"))
    write_rgb(out("b.denoised.png"), rt.denoise_sampler(carried, aov_b, smp_b))
    cnt = carried.download()[2]
    carried.free()
    hit = int(np.isfinite(aov_b["depth"]).sum())
    print(json.dumps({"model": a.model, "scene": a.scene, "width": W, "height": H, "spp": a.spp, "spp2": a.spp2,
                      "hit_pixels": hit, "kept_pixels": stats["kept_pixels"],
                      "kept_of_hit": round(stats["kept_pixels"] / max(hit, 1), 4),
                      "mean_count": round(float(cnt.mean()), 3), "out_dir": a.out_dir}))


def bench(a):
    L = rt.lib()
    gpu_timing.require_device("model_frames")
    timer = gpu_timing.Timer()
    stream = timer.stream
    run = helpers.GpuRun(a.scene)
    sizes = {"equirect": (1920, 960), "fisheye": (1920, 1080), "pinhole": (1920, 1080), "ortho": (1920, 1080)}
    n_max = 1920 * 1080

    def aov_buffers():
        return [rt.DeviceArray(n_max * per, dtype) for per, dtype in ((1, f32), (3, f32), (3, f32), (1, np.int32))]

    aov_a, aov_b, aov_c = aov_buffers(), aov_buffers(), aov_buffers()  # camera A, camera B, the composition's
    d_rays, d_rgb = rt.DeviceArray((n_max, 6), f32), rt.DeviceArray((n_max, 3), f32)
    d_hits, d_surf = rt.DeviceArray(n_max, rt.RAY_HIT), rt.DeviceArray(n_max, rt.RAY_SURFACE)
    g, g_out = rt.GBuffer(1920, 1080), rt.GBuffer(1920, 1080)

    def read(d, count, dtype):
        """the first `count` values of a device array"""
        return rt.DeviceArray.at(d, count, dtype).read()

    variants = {}  # name -> Variant
    for kind, (W, H) in sizes.items():
        n = W * H
        sa, sb = model_sampler(run, kind, W, H), model_sampler(run, kind, W, H, (0.04, 0.03, 0.02))
        rp = lambda x: (x[0], x[1], x[3])  # noqa: E731  (depth, normal, triangle)
        fields = {"sampler": kind, "width": W, "height": H}

        def prepare(sa=sa, sb=sb, n=n):
            """camera A's frame (1 spp) and both cameras' guides, outside every timed span"""
            rt.sample_paths_device(run.dev, sa, g.g.random_numbers, n, g.g.frame_buffer, g.g.squared_luminance,
                                   g.g.sample_count, samples=1)
            rt.sample_aov_device(run.dev, sa, n, aov_a)
            rt.sample_aov_device(run.dev, sb, n, aov_b)

        if kind in ("equirect", "fisheye"):
            def fused(sa=sa, n=n):
                rt.sample_aov_device(run.dev, sa, n, aov_c, stream=stream.value)

            def composed(sa=sa, n=n):
                s = sa.struct()
                rt.check(L.rt_sampler_rays(ctypes.byref(s), None, n, d_rays, stream))
                rt.trace_rays_device(run.dev, d_rays, n, d_hits, d_surf, stream=stream.value)
            variants[f"sample_aov/{kind}/rt_sample_aov"] = Variant("sample_aov/" + kind, prepare, fused, fields)
            variants[f"sample_aov/{kind}/rays+trace"] = Variant("sample_aov/" + kind, prepare, composed, fields)
        if kind == "equirect":
            def dn_sampler(sa=sa):
                rt.denoise_sampler_device(g.g, aov_a[:3], sa, d_rgb, stream=stream.value)

            def dn_plain(W=W, H=H):
                rt.denoise_device(g.g, aov_a[:3], W, H, d_rgb, stream=stream.value)
            variants["denoise/equirect/rt_denoise_sampler"] = Variant("denoise/equirect", prepare, dn_sampler, fields)
            variants["denoise/equirect/rt_denoise"] = Variant("denoise/equirect", prepare, dn_plain, fields)

        def rp_sampler(sa=sa, sb=sb):
            rt.reproject_sampler_device(g.g, rp(aov_a), sa, rp(aov_b), sb, g_out.g, stream=stream.value)

        def rp_plain(sa=sa, sb=sb, W=W, H=H):
            rt.reproject_device(g.g, rp(aov_a), sa.camera, rp(aov_b), sb.camera, W, H, g_out.g, stream=stream.value)
        variants[f"reproject/{kind}/rt_reproject_sampler"] = Variant("reproject/" + kind, prepare, rp_sampler, fields)
        variants[f"reproject/{kind}/rt_reproject"] = Variant("reproject/" + kind, prepare, rp_plain, fields)

    # the fused AOV pass must be the composition before the two are compared
    for kind in ("equirect", "fisheye"):
        _, prepare, fused, fields = variants[f"sample_aov/{kind}/rt_sample_aov"]
        n = fields["width"] * fields["height"]
        variants[f"sample_aov/{kind}/rays+trace"].fn()
        fused()
        timer.synchronize()
        surf = read(d_surf, n, rt.RAY_SURFACE)
        hits = read(d_hits, n, rt.RAY_HIT)
        for got, want, what in ((read(aov_c[0], n, f32), surf["t"], "depth"), (read(aov_c[1], 3 * n, f32), surf["normal"], "normal"),
                                (read(aov_c[2], 3 * n, f32), surf["albedo"], "albedo"),
                                (read(aov_c[3], n, np.int32), hits["triangle"], "triangle")):
            want = np.ascontiguousarray(want).reshape(-1)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"{kind}: {what} differs"

    # one size at a time: its frame and guides are made once, its variants alternate
    times = {}
    for kind in sizes:
        names = [name for name in variants if name.split("/")[1] == kind]
        variants[names[0]].prepare()
        rt.check(L.rt_synchronize())
        times.update(gpu_timing.interleaved(names, lambda name: timer.span(variants[name].fn)[0], a.warmup, a.reps))
    records = []
    for name, (group, _, _, fields) in variants.items():
        med = float(np.median(times[name]))
        base = float(np.median(times[[x for x in variants if variants[x].group == group][-1]]))
        records.append(dict(scene=a.scene, call=name.split("/")[0], variant=name.split("/")[2], **fields,
                            **gpu_timing.summary(times[name], 4), time_over_baseline=round(med / base, 4)))
    gpu_timing.write_lines(a.out, records)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bench", action="store_true")
    ap.add_argument("--scene", default=None)
    ap.add_argument("--model", default="equirect", choices=["pinhole", "equirect", "fisheye", "ortho"])
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--height", type=int, default=256)
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--spp2", type=int, default=4)
    ap.add_argument("--move", type=float, nargs=3, default=(0.04, 0.03, 0.02), metavar=("DX", "DZ", "DYAW"))
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "model_frames", "frames"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "model_frames", "bench.jsonl"))
    a = ap.parse_args()
    a.move = tuple(a.move)
    if a.scene is None:
        a.scene = "room2m" if a.bench else "room_small"
    rt.check(rt.lib().rt_set_device(0))
    bench(a) if a.bench else flow(a)


if __name__ == "__main__":
    main()
