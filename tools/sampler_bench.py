"""rt_sample_paths against the ways to do without it, on the 2M-triangle bench
scene (room2m) at 1920x1080, 4 samples per pixel, for the PINHOLE and the
EQUIRECT sampler of the scene's camera:

  fused     one rt_sample_paths(samples = 4): every lane draws its element's
            next ray in the iteration its previous path ended in;
  unfused   4 x (rt_sampler_rays + rt_trace_paths(samples = 1)): the rays of
            each sample go through a 50 MB device buffer;
  uploaded  4 x (the sample's rays copied from host memory + rt_trace_paths):
            what a caller did before the samplers existed (the rays are made
            ahead of the timed span by rt_sampler_rays_host, which is kind to
            that caller: only the copy is timed).

Each launch runs between two device events on one stream and ends in a
synchronise; a host clock around the same span is recorded beside it.  The RNG
states are put back before every launch, outside the timed span, so every
launch of a variant does the same work.  After a warm-up of every variant the
variants alternate for --reps rounds in one process.  One JSON line per variant
in --out: median, min, max and the spread (max - min) / median of the event
timings, the host-clock median, Mpaths/s, and time over the unfused variant.
Before any timing the three variants of a kind must agree bit for bit in
radiance, squared luminance and RNG state.

usage: python tools/sampler_bench.py [--scene room2m] [--reps 10] [--warmup 2]
                                     [--width 1920 --height 1080] [--out FILE]
"""
import argparse
import ctypes
import os

import numpy as np

import gpu_timing
from gpu_timing import ROOT

import helpers  # noqa: E402
import rt  # noqa: E402

f32 = np.float32
SAMPLES = 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="room2m")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "samplers", "bench.jsonl"))
    a = ap.parse_args()
    W, H = a.width, a.height
    n = W * H

    L = rt.lib()
    gpu_timing.require_device("sampler_bench")
    timer = gpu_timing.Timer()
    run = helpers.GpuRun(a.scene)
    seeds = rt.seeds(n)
    d_rng, d_rad, d_sq = rt.DeviceArray(n, np.uint32), rt.DeviceArray((n, 3), f32), rt.DeviceArray(n, f32)
    d_cnt, d_rays = rt.DeviceArray(n, np.int32), rt.DeviceArray((n, 6), f32)
    kinds = {"pinhole": rt.Sampler("pinhole", W, H, run.camera), "equirect": rt.Sampler("equirect", W, H, run.camera)}
    host_rays = {kind: [] for kind in kinds}  # the uploaded variant's (rays, states after the draws) per sample
    variants = [(kind, how) for kind in kinds for how in ("fused", "unfused", "uploaded")]

    def launch(v):
        kind, how = v
        smp = kinds[kind]
        d_rng.upload(seeds)

        def work():
            if how == "fused":
                rt.sample_paths_device(run.dev, smp, d_rng, n, d_rad, d_sq, d_cnt, samples=SAMPLES, stream=timer.s)
                return
            for k in range(SAMPLES):
                if how == "unfused":
                    s = smp.struct()
                    rt.check(L.rt_sampler_rays(ctypes.byref(s), d_rng, n, d_rays, timer.stream))
                else:
                    # the host's rays of this sample, and the states after their draws (4 B per pixel more), so
                    # that this variant computes the fused one's result bit for bit (the bare copies: this is timed)
                    rt.check(L.rt_upload(d_rays, host_rays[kind][k][0].ctypes.data, 24 * n))
                    rt.check(L.rt_upload(d_rng, host_rays[kind][k][1].ctypes.data, 4 * n))
                rt.trace_paths_device(run.dev, d_rays, d_rng, n, d_rad, d_sq, samples=1, accumulate=k > 0,
                                      stream=timer.s)
        return timer.span(work)

    def results():
        return [d_rad.read(), d_sq.read(), d_rng.read()]

    # the uploaded variant's rays, made ahead of time: sample k's start from the states sample k - 1's paths left
    for kind, smp in kinds.items():
        d_rng.upload(seeds)
        for k in range(SAMPLES):
            rays, after = rt.sampler_rays_host(smp, d_rng.read())
            host_rays[kind].append((rays, after))
            d_rays.upload(rays)
            d_rng.upload(after)
            rt.trace_paths_device(run.dev, d_rays, d_rng, n, d_rad, d_sq, samples=1, accumulate=k > 0)

    # the three variants of a kind must agree before they are compared
    for kind in kinds:
        launch((kind, "fused"))
        want = results()
        for how in ("unfused", "uploaded"):
            launch((kind, how))
            for arr, ref, what in zip(results(), want, ("radiance", "sq", "rng")):
                assert np.array_equal(arr.view(np.uint32), ref.view(np.uint32)), f"{kind} {how}: {what} differs from fused"
        assert (want[0] != 0).any(axis=1).mean() > 0.10

    times = gpu_timing.interleaved(variants, launch, a.warmup, a.reps)
    records = []
    for v in variants:
        t = [x[0] for x in times[v]]
        med = float(np.median(t))
        base = float(np.median([x[0] for x in times[(v[0], "unfused")]]))
        records.append({"scene": a.scene, "sampler": v[0], "variant": v[1], "width": W, "height": H, "samples": SAMPLES,
                        "paths": n * SAMPLES, **gpu_timing.summary(t, 3),
                        "host_ms_median": round(float(np.median([x[1] for x in times[v]])), 3),
                        "mpaths_per_s_median": round(n * SAMPLES / med / 1e3, 2),
                        "time_over_unfused": round(med / base, 4), "equals_fused_bitwise": True})
    gpu_timing.write_lines(a.out, records)


if __name__ == "__main__":
    main()
