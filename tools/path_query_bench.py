"""rt_trace_paths against rt_render on the 2M-triangle bench scene (room2m):

  (a) camera      the jittered camera samples of one pass of a 1920x1080 frame
                  (tests/path_query_ref.camera_samples on the frame's seeds) —
                  the work of one rt_render pass, ray for ray;
  (b) incoherent  as many rays with seeded origins in the scene box and seeded
                  unit directions.

One sample per ray.  rt_trace_paths on both sets and rt_render of one
unchained pass on the same frame (RT_KERNEL_MEGA, the bounded megakernel, and
the default wavefront) are timed over --reps launches between device events,
interleaved in one process after a warm-up of every variant; the RNG states
are put back before every launch (outside the timed span), so every launch of
a variant does the same work.  One JSON line per variant in --out: median,
min, max and the spread (max - min) / median of the timings, Mpaths/s, and for
the query the counted work of one extra launch (trace_ray calls per path, the
longest path).  Before any timing the query on set (a) must reproduce the
megakernel's frame_buffer, squared_luminance and random_numbers bit for bit.

usage: python tools/path_query_bench.py [--scene room2m] [--reps 20] [--warmup 3]
                                        [--width 1920 --height 1080] [--out FILE]
"""
import argparse
import os

import numpy as np

import gpu_timing
from gpu_timing import ROOT

import helpers  # noqa: E402
import path_query_ref  # noqa: E402
import rt  # noqa: E402

f32 = np.float32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="room2m")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "path_query", "bench.jsonl"))
    a = ap.parse_args()
    W, H = a.width, a.height
    n = W * H

    gpu_timing.require_device("path_query_bench")
    timer = gpu_timing.Timer()
    run = helpers.GpuRun(a.scene)
    gbuf = rt.GBuffer(W, H)
    gbuf_rng = gbuf.array("random_numbers")
    seeds = gbuf_rng.read()
    cam_rays, cam_rng = path_query_ref.camera_samples(np.asarray(run.camera.as_list(), f32), W, H, seeds)
    raw, ntris = run.host.triangles_bytes()
    verts = np.frombuffer(raw, np.uint8).reshape(ntris, rt.TRIANGLE_BYTES)[:, :36].copy().view(f32).reshape(-1, 3)
    g = np.random.default_rng(8)
    d = g.normal(size=(n, 3))
    inc_rays = np.concatenate([g.uniform(verts.min(axis=0), verts.max(axis=0), (n, 3)),
                               d / np.linalg.norm(d, axis=1)[:, None]], axis=1).astype(f32)
    sets = {"camera": (cam_rays, cam_rng), "incoherent": (inc_rays, seeds)}

    bufs = {k: {"rays": rt.DeviceArray(r), "rng": rt.DeviceArray(s), "rad": rt.DeviceArray((n, 3), f32, zero=True),
                "sq": rt.DeviceArray(n, f32, zero=True), "stats": rt.DeviceArray(5, np.uint64, zero=True)}
            for k, (r, s) in sets.items()}
    variants = [("rt_trace_paths", "camera"), ("rt_trace_paths", "incoherent"), ("rt_render mega", "camera"),
                ("rt_render wavefront", "camera")]

    def launch(v, stats=False):
        call, name = v
        if call == "rt_trace_paths":  # (the launch's RNG states: the set's own)
            b = bufs[name]
            b["rng"].upload(sets[name][1])

            def work():
                rt.trace_paths_device(run.dev, b["rays"], b["rng"], n, b["rad"], b["sq"], stream=timer.s,
                                      stats_ptr=b["stats"] if stats else None)
        else:
            gbuf_rng.upload(seeds)
            opt = rt.options(W, H, 1, adaptive=False, stream=timer.s,
                             kernel=rt.KERNEL_MEGA if call == "rt_render mega" else rt.KERNEL_WAVEFRONT)

            def work():
                rt.render(run.dev, gbuf, run.camera, 0, opt)
        ms = timer.span(work)[0]
        rt.join()
        return ms

    # the query on the camera samples must be the megakernel's pass before the two are compared
    launch(("rt_render mega", "camera"))
    fb, sq, cnt, rng = gbuf.download()
    assert (cnt == 1).all()
    counted = {}
    for name in sets:
        b = bufs[name]
        launch(("rt_trace_paths", name), stats=True)
        counted[name] = dict(zip(rt.PATH_STATS, (int(x) for x in b["stats"].read())))
        assert counted[name]["rays"] == n and counted[name]["paths"] == n
    got = [bufs["camera"][key].read() for key in ("rad", "sq", "rng")]
    for arr, want, what in zip(got, (fb, sq, rng), ("radiance", "sq", "rng")):
        assert np.array_equal(arr.view(np.uint32), want.view(np.uint32)), f"{what} differs from the megakernel's pass"

    times = gpu_timing.interleaved(variants, launch, a.warmup, a.reps)
    base = float(np.median(times[("rt_render mega", "camera")]))
    records = []
    for v in variants:
        med = float(np.median(times[v]))
        rec = {"scene": a.scene, "call": v[0], "set": v[1], "paths": n, **gpu_timing.summary(times[v], 4),
               "mpaths_per_s_median": round(n / med / 1e3, 2), "time_over_megakernel": round(med / base, 3)}
        if v[0] == "rt_trace_paths":
            c = counted[v[1]]
            rec["trace_calls_per_path"] = round(c["trace_calls"] / n, 3)
            rec["longest_path"] = c["max_depth"]
            if v[1] == "camera":
                rec["equals_megakernel_pass_bitwise"] = True
        records.append(rec)
    gpu_timing.write_lines(a.out, records)


if __name__ == "__main__":
    main()
