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
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "isaklm-raytracer_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402

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
    if not helpers.gpu_has_device():
        raise SystemExit("sampler_bench: no HIP device (nothing is measured without one)")
    rt.check(L.rt_set_device(0))
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipEventElapsedTime.argtypes = [ctypes.POINTER(ctypes.c_float), ctypes.c_void_p, ctypes.c_void_p]
    hip.hipEventRecord.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    hip.hipEventSynchronize.argtypes = [ctypes.c_void_p]
    stream, e0, e1 = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
    assert hip.hipStreamCreate(ctypes.byref(stream)) == 0
    assert hip.hipEventCreate(ctypes.byref(e0)) == 0 and hip.hipEventCreate(ctypes.byref(e1)) == 0

    run = helpers.GpuRun(a.scene)
    seeds = rt.seeds(n)

    def dev(nbytes):
        p = ctypes.c_void_p()
        rt.check(L.rt_device_alloc(ctypes.byref(p), max(nbytes, 16)))
        return p

    d_rng, d_rad, d_sq, d_cnt, d_rays = dev(4 * n), dev(12 * n), dev(4 * n), dev(4 * n), dev(24 * n)
    kinds = {"pinhole": rt.Sampler("pinhole", W, H, run.camera), "equirect": rt.Sampler("equirect", W, H, run.camera)}
    host_rays = {kind: [] for kind in kinds}  # the uploaded variant's (rays, states after the draws) per sample
    variants = [(kind, how) for kind in kinds for how in ("fused", "unfused", "uploaded")]

    def launch(v):
        kind, how = v
        smp = kinds[kind]
        rt.check(L.rt_upload(d_rng, seeds.ctypes.data, 4 * n))
        t0 = time.perf_counter()
        assert hip.hipEventRecord(e0, stream) == 0
        if how == "fused":
            rt.sample_paths_device(run.dev, smp, d_rng, n, d_rad, d_sq, d_cnt, samples=SAMPLES, stream=stream.value)
        else:
            for k in range(SAMPLES):
                if how == "unfused":
                    s = smp.struct()
                    rt.check(L.rt_sampler_rays(ctypes.byref(s), d_rng, n, d_rays, stream))
                else:
                    # the host's rays of this sample, and the states after their draws (4 B per pixel more), so
                    # that this variant computes the fused one's result bit for bit
                    rt.check(L.rt_upload(d_rays, host_rays[kind][k][0].ctypes.data, 24 * n))
                    rt.check(L.rt_upload(d_rng, host_rays[kind][k][1].ctypes.data, 4 * n))
                rt.trace_paths_device(run.dev, d_rays, d_rng, n, d_rad, d_sq, samples=1, accumulate=k > 0,
                                      stream=stream.value)
        assert hip.hipEventRecord(e1, stream) == 0
        assert hip.hipEventSynchronize(e1) == 0
        wall = (time.perf_counter() - t0) * 1e3
        ms = ctypes.c_float()
        assert hip.hipEventElapsedTime(ctypes.byref(ms), e0, e1) == 0
        return ms.value, wall

    def results():
        out = [np.zeros((n, 3), f32), np.zeros(n, f32), np.zeros(n, np.uint32)]
        for arr, p in zip(out, (d_rad, d_sq, d_rng)):
            rt.check(L.rt_download(arr.ctypes.data, p, arr.nbytes))
        return out

    # the uploaded variant's rays, made ahead of time: sample k's start from the states sample k - 1's paths left
    for kind, smp in kinds.items():
        rt.check(L.rt_upload(d_rng, seeds.ctypes.data, 4 * n))
        for k in range(SAMPLES):
            st = np.zeros(n, np.uint32)
            rt.check(L.rt_download(st.ctypes.data, d_rng, 4 * n))
            rays, after = rt.sampler_rays_host(smp, st)
            host_rays[kind].append((rays, after))
            rt.check(L.rt_upload(d_rays, rays.ctypes.data, 24 * n))
            rt.check(L.rt_upload(d_rng, after.ctypes.data, 4 * n))
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

    for _ in range(a.warmup):
        for v in variants:
            launch(v)
    times = {v: [] for v in variants}
    for _ in range(a.reps):
        for v in variants:
            times[v].append(launch(v))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for v in variants:
            t = np.array([x[0] for x in times[v]])
            wall = np.array([x[1] for x in times[v]])
            med = float(np.median(t))
            base = float(np.median([x[0] for x in times[(v[0], "unfused")]]))
            rec = {"scene": a.scene, "sampler": v[0], "variant": v[1], "width": W, "height": H, "samples": SAMPLES,
                   "paths": n * SAMPLES, "reps": a.reps, "ms_median": round(med, 3), "ms_min": round(float(t.min()), 3),
                   "ms_max": round(float(t.max()), 3), "spread": round(float(t.max() - t.min()) / med, 4),
                   "host_ms_median": round(float(np.median(wall)), 3),
                   "mpaths_per_s_median": round(n * SAMPLES / med / 1e3, 2), "time_over_unfused": round(med / base, 4),
                   "equals_fused_bitwise": True}
            line = json.dumps(rec)
            print(line, flush=True)
            f.write(line + "\n")


if __name__ == "__main__":
    main()
