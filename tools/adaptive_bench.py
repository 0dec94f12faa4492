"""rt_sample_paths_adaptive and rt_convergence on the 2M-triangle bench scene
(room2m) at 1920x1080, up to 64 samples per pixel under min_samples 16 and
tolerance 0.05, for the PINHOLE and the EQUIRECT sampler of the scene's camera:

  fixed        rt_sample_paths(samples = 64): every pixel takes every sample;
  adaptive     rt_sample_paths_adaptive(samples = 64): a pixel stops where the
               adaptive test stops it;
  render       (pinhole) rt_render(passes = 64, adaptive = 1) on a G_Buffer
               with the same seeds — the frame the adaptive pinhole call
               equals bit for bit (checked before any timing), joined;
  converged    the adaptive call again, accumulating onto its own frame under
               a tolerance nothing exceeds: every element reads its records,
               fails the test and is done — the cost of asking a finished frame
               for more;
  convergence  rt_convergence (statistics and the relative-error map) of the
               adaptive frame.

Each launch runs between two device events on one stream and ends in a
synchronise; a host clock around the same span is recorded beside it.  The RNG
states (and for `converged` / `convergence` the frame) are put in place before
every launch, outside the timed span, so every launch of a variant does the
same work.  After a warm-up of every variant the variants alternate for --reps
rounds in one process.  One JSON line per variant in --out: median, min, max
and the spread (max - min) / median of the event timings, the host-clock
median, the samples actually taken, and time over the kind's fixed call.

usage: python tools/adaptive_bench.py [--scene room2m] [--reps 10] [--warmup 1] [--samples 64]
                                      [--min-samples 16] [--tolerance 0.05]
                                      [--width 1920 --height 1080] [--out FILE]
"""
import argparse
import os

import numpy as np

import gpu_timing
from gpu_timing import ROOT

import helpers  # noqa: E402
import rt  # noqa: E402

f32 = np.float32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="room2m")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--min-samples", type=int, default=16)
    ap.add_argument("--tolerance", type=float, default=0.05)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adaptive", "bench.jsonl"))
    a = ap.parse_args()
    W, H = a.width, a.height
    n = W * H
    test = (a.min_samples, a.tolerance)

    gpu_timing.require_device("adaptive_bench")
    timer = gpu_timing.Timer()
    run = helpers.GpuRun(a.scene)
    seeds = rt.seeds(n)
    gb = rt.GBuffer(W, H)  # every variant works on this G_Buffer's four arrays
    g = gb.g
    d_err, d_cstats, d_pstats = rt.DeviceArray(n, f32), rt.DeviceArray(4, np.uint64), rt.DeviceArray(5, np.uint64)
    kinds = {"pinhole": rt.Sampler("pinhole", W, H, run.camera), "equirect": rt.Sampler("equirect", W, H, run.camera)}
    variants = [(kind, how) for kind in kinds for how in ("fixed", "adaptive", "render", "converged", "convergence")
                if not (kind != "pinhole" and how == "render")]
    frames = {}  # kind -> the adaptive frame (fb, sq, count, rng) on the host
    taken = {}   # variant -> samples taken by one launch

    def sample(smp, **more):
        rt.sample_paths_device(run.dev, smp, g.random_numbers, n, g.frame_buffer, g.squared_luminance, g.sample_count,
                               samples=a.samples, stream=timer.s, stats_ptr=d_pstats, **more)

    def launch(v):
        kind, how = v
        smp = kinds[kind]
        if how in ("converged", "convergence"):
            gb.upload(*frames[kind])
        else:
            gb.array("random_numbers").upload(seeds)
        d_pstats.zero()
        d_cstats.zero()

        def work():
            if how == "fixed":
                sample(smp)
            elif how == "adaptive":
                sample(smp, adaptive=test)
            elif how == "converged":
                sample(smp, accumulate=True, adaptive=(a.min_samples, 1e9))
            elif how == "convergence":
                rt.convergence_device(g.frame_buffer, g.squared_luminance, g.sample_count, n, a.min_samples, a.tolerance,
                                      d_err, d_cstats, stream=timer.s)
            else:
                opt = rt.options(W, H, a.samples, adaptive=True, min_samples=a.min_samples, tolerance=a.tolerance,
                                 kernel=rt.KERNEL_WAVEFRONT, stream=timer.s)
                rt.render(run.dev, gb, run.camera, 0, opt)
                rt.join(timer.s)
        ms, wall = timer.span(work)
        taken[v] = int(d_pstats.read()[1])
        return ms, wall

    # before any timing: the adaptive frames, and the pinhole one against rt_render's
    for kind in kinds:
        launch((kind, "adaptive"))
        frames[kind] = gb.download()
        assert taken[(kind, "adaptive")] == int(frames[kind][2].sum())
        launch((kind, "converged"))
        assert taken[(kind, "converged")] == 0
        for arr, ref, what in zip(gb.download(), frames[kind], ("fb", "sq", "count", "rng")):
            assert np.array_equal(arr.view(np.uint32), ref.view(np.uint32)), f"{kind}: an all-converged call changed {what}"
    launch(("pinhole", "render"))
    for arr, ref, what in zip(gb.download(), frames["pinhole"], ("fb", "sq", "count", "rng")):
        assert np.array_equal(arr.view(np.uint32), ref.view(np.uint32)), f"pinhole adaptive: {what} differs from rt_render"
    taken[("pinhole", "render")] = int(frames["pinhole"][2].sum())

    times = gpu_timing.interleaved(variants, launch, a.warmup, a.reps)
    taken[("pinhole", "render")] = int(frames["pinhole"][2].sum())
    records = []
    for v in variants:
        t = [x[0] for x in times[v]]
        med = float(np.median(t))
        base = float(np.median([x[0] for x in times[(v[0], "fixed")]]))
        cnt = frames[v[0]][2]
        rec = {"scene": a.scene, "sampler": v[0], "variant": v[1], "width": W, "height": H, "samples": a.samples,
               "min_samples": a.min_samples, "tolerance": a.tolerance, **gpu_timing.summary(t, 3),
               "host_ms_median": round(float(np.median([x[1] for x in times[v]])), 3),
               "samples_taken": taken[v], "mean_samples_per_pixel": round(taken[v] / n, 3),
               "time_over_fixed": round(med / base, 4)}
        if v[1] == "adaptive":
            rec["pixels_stopped_at_min"] = int((cnt == a.min_samples).sum())
            rec["pixels_never_stopped"] = int((cnt == a.samples).sum())
        records.append(rec)
    gpu_timing.write_lines(a.out, records)


if __name__ == "__main__":
    main()
