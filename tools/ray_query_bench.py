"""Rays per second of rt_trace_rays on the 2M-triangle bench scene (room2m):

  (a) camera    the 1920x1080 rt_camera_rays set (coherent primary rays);
  (b) bounce    an incoherent set: from (a)'s hit points, seeded uniform
                directions on the sphere;

each in both traversals (bounded / kd).  After a warm-up every variant is
timed over --reps launches between device events, the variants interleaved
in one process (so clock and thermal drift hit them alike); the result is
one JSON line per variant (median, min, max ms and Mrays/s) in --out.

The same script decided the kernel's refill scheme ("Ray queries"):
a temporary build that also held a parked per-lane refill variant was timed
as a third column, profiles/ray_query/refill_experiment_lockstep_vs_park.jsonl.

usage: python tools/ray_query_bench.py [--scene room2m] [--reps 20] [--warmup 3]
                                       [--width 1920 --height 1080] [--out FILE]
"""
import argparse
import os

import numpy as np

import gpu_timing
from gpu_timing import ROOT

import helpers  # noqa: E402
import rt  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="room2m")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ray_query", "ray_query_bench.jsonl"))
    a = ap.parse_args()

    gpu_timing.require_device("ray_query_bench")
    timer = gpu_timing.Timer()
    run = helpers.GpuRun(a.scene)
    cam_rays = rt.camera_rays(run.camera, a.width, a.height)
    hits, surf = rt.trace_rays(run.dev, cam_rays, surface=True)
    ok = hits["triangle"] >= 0
    g = np.random.default_rng(5)
    d = g.normal(size=(int(ok.sum()), 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    bounce = np.concatenate([surf["position"][ok], d.astype(np.float32)], axis=1).astype(np.float32)
    sets = {"camera": cam_rays, "bounce": bounce}

    bufs = {k: (rt.DeviceArray(v), rt.DeviceArray(len(v), rt.RAY_HIT, zero=True), len(v)) for k, v in sets.items()}
    variants = []
    for set_name in sets:
        for trav_name, trav in (("bounded", rt.TRAVERSAL_BOUNDED), ("kd", rt.TRAVERSAL_KD)):
            variants.append((set_name, trav_name, trav, "lockstep"))

    def launch(v):
        set_name, _, trav, _ = v
        rays, out, cnt = bufs[set_name]
        return timer.span(lambda: rt.trace_rays_device(run.dev, rays, cnt, out, traversal=trav, stream=timer.s))[0]

    # the traversals must agree with each other before they are compared
    check = {}
    for v in variants:
        launch(v)
        h = bufs[v[0]][1].read()
        key = v[0]
        if key in check:
            assert np.array_equal(check[key].view(np.uint32), h.view(np.uint32)), v
        check[key] = h
    times = gpu_timing.interleaved(variants, launch, a.warmup, a.reps)
    records = []
    for v in variants:
        cnt = bufs[v[0]][2]
        s = gpu_timing.summary(times[v], 4)
        records.append({"scene": a.scene, "set": v[0], "rays": cnt, "traversal": v[1], "refill": v[3], **s,
                        "mrays_per_s_median": round(cnt / float(np.median(times[v])) / 1e3, 1),
                        "hit_fraction": round(float((check[v[0]]["triangle"] >= 0).mean()), 4)})
    gpu_timing.write_lines(a.out, records)


if __name__ == "__main__":
    main()
