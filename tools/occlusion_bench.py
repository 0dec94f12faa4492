"""rt_occluded against rt_trace_rays (hits only) on the same rays, on the
2M-triangle bench scene (room2m), ray sets built from the first hits of a
1920x1080 camera:

  (a) camera   the rt_camera_rays set, tmax = +inf;
  (b) shadow   from the first-hit points towards seeded points on the emissive
               triangles: unit direction, tmax = distance * (1 - 2^-10);
  (c) short    from the first-hit points in seeded directions of the hemisphere
               around the hit's normal, tmax = 2 % of the scene box's diagonal.

After a warm-up of every variant the variants are timed over --reps launches
between device events, interleaved in one process (clock and thermal drift
hit them alike).  One JSON line per (set, call) in --out: median, min, max
and the spread (max - min) / median of the timings, Mrays/s, the occluded /
hit fractions; the rt_occluded line also carries its speed-up over
rt_trace_rays and whether it kept the condition "not slower than
rt_trace_rays by more than the spread of rt_trace_rays' own timings".  Before
any timing the two calls must agree: with tmax = +inf rt_occluded is
rt_trace_rays' hit flag on every set.

--count-lib PATH: a counting build of the library (-DRQ_COUNT_EARLY=1,
tools/mkvariant.sh), run in a child process: the share of rays the capped
s_min query answers alone is added to each set's rt_occluded line
("early_share").  Without it the share is reported as null (not measured).

usage: python tools/occlusion_bench.py [--scene room2m] [--reps 20] [--warmup 3]
                                       [--width 1920 --height 1080] [--out FILE] [--count-lib PATH]
"""
import argparse
import contextlib
import json
import os
import subprocess
import sys

import numpy as np

import gpu_timing
from gpu_timing import ROOT

import helpers  # noqa: E402
import rt  # noqa: E402

f32 = np.float32


def ray_sets(run, width, height):
    """{name: (rays (n, 6) float32, tmax (n,) float32 or None)}"""
    cam_rays = rt.camera_rays(run.camera, width, height)
    hits, surf = rt.trace_rays(run.dev, cam_rays, surface=True)
    ok = hits["triangle"] >= 0
    pos, nrm = surf["position"][ok].astype(np.float64), surf["normal"][ok].astype(np.float64)
    n = len(pos)
    g = np.random.default_rng(6)
    raw, ntris = run.host.triangles_bytes()
    tris = np.frombuffer(raw, np.uint8).reshape(ntris, rt.TRIANGLE_BYTES)
    emit = tris[:, 108:120].copy().view(f32)
    lights = np.nonzero((emit > 0).any(axis=1))[0]
    assert len(lights) > 0, "the scene has no emissive triangle"
    p = tris[lights, :36].copy().view(f32).reshape(-1, 3, 3).astype(np.float64)
    pick = g.integers(0, len(lights), n)
    b1, b2 = g.random(n), g.random(n)
    flip = b1 + b2 > 1
    b1[flip], b2[flip] = 1 - b1[flip], 1 - b2[flip]
    target = p[pick, 0] + b1[:, None] * (p[pick, 1] - p[pick, 0]) + b2[:, None] * (p[pick, 2] - p[pick, 0])
    d = target - pos
    dist = np.linalg.norm(d, axis=1)
    keep = dist > 1e-6
    shadow = np.concatenate([pos[keep], d[keep] / dist[keep, None]], axis=1).astype(f32)
    shadow_tmax = (dist[keep] * (1.0 - 2.0 ** -10)).astype(f32)
    h = g.normal(size=(n, 3))
    h /= np.linalg.norm(h, axis=1)[:, None]
    h[np.einsum("ij,ij->i", h, nrm) < 0] *= -1.0  # into the hemisphere around the normal
    short = np.concatenate([pos, h], axis=1).astype(f32)
    verts = tris[:, :36].copy().view(f32).reshape(-1, 3)  # the scene box = the vertices' box
    diag = float(np.linalg.norm(verts.max(axis=0).astype(np.float64) - verts.min(axis=0)))
    short_tmax = np.full(n, 0.02 * diag, f32)
    return {"camera": (cam_rays, None), "shadow": (shadow, shadow_tmax), "short": (short, short_tmax)}


def count_early(a):
    """child mode (the counting build is loaded through ISAKLM_RT_LIB_OVERRIDE): prints {set: early share}"""
    gpu_timing.require_device("occlusion_bench")
    run = helpers.GpuRun(a.scene)
    out = {}
    for name, (rays, tmax) in ray_sets(run, a.width, a.height).items():
        with contextlib.ExitStack() as stack:
            put = stack.enter_context
            d_rays, d_out = put(rt.DeviceArray(rays)), put(rt.DeviceArray(len(rays), np.uint8))
            d_st = put(rt.DeviceArray(4, np.uint64, zero=True))
            d_tmax = put(rt.DeviceArray(tmax)) if tmax is not None else None
            rt.occluded_device(run.dev, d_rays, d_tmax, len(rays), d_out, stats_ptr=d_st)
            st = d_st.read()
        assert int(st[0]) == len(rays)
        out[name] = round(int(st[3]) / len(rays), 4)
    print("EARLY " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="room2m")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "occlusion", "bench.jsonl"))
    ap.add_argument("--count-lib", default=None)
    ap.add_argument("--count-child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.count_child:
        return count_early(a)

    early = None
    if a.count_lib:  # a fresh process: this one loads the shipped library
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--count-child", "--scene", a.scene, "--width",
                            str(a.width), "--height", str(a.height)], capture_output=True, text=True,
                           env=dict(os.environ, ISAKLM_RT_LIB_OVERRIDE=os.path.abspath(a.count_lib)))
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("EARLY ")]
        if r.returncode != 0 or not lines:
            sys.exit("the counting build's run failed:\n" + r.stdout[-2000:] + r.stderr[-2000:])
        early = json.loads(lines[-1][6:])

    gpu_timing.require_device("occlusion_bench")
    timer = gpu_timing.Timer()
    run = helpers.GpuRun(a.scene)
    sets = ray_sets(run, a.width, a.height)
    bufs = {}
    for k, (rays, tmax) in sets.items():
        bufs[k] = {"rays": rt.DeviceArray(rays), "tmax": rt.DeviceArray(tmax) if tmax is not None else None,
                   "n": len(rays), "hits": rt.DeviceArray(len(rays), rt.RAY_HIT, zero=True),
                   "occ": rt.DeviceArray(len(rays), np.uint8, zero=True)}
    variants = [(k, call) for k in sets for call in ("rt_trace_rays", "rt_occluded")]

    def launch(v, tmax=True):
        b = bufs[v[0]]
        if v[1] == "rt_trace_rays":
            return timer.span(lambda: rt.trace_rays_device(run.dev, b["rays"], b["n"], b["hits"], stream=timer.s))[0]
        return timer.span(lambda: rt.occluded_device(run.dev, b["rays"], b["tmax"] if tmax else None, b["n"], b["occ"],
                                                     stream=timer.s))[0]

    # the two calls must agree before they are compared: without a tmax rt_occluded is the hit flag
    frac = {}
    for k in sets:
        b = bufs[k]
        launch((k, "rt_trace_rays"))
        launch((k, "rt_occluded"), tmax=False)
        h, o = b["hits"].read(), b["occ"].read()
        assert np.array_equal(o, (h["triangle"] >= 0).astype(np.uint8)), k
        launch((k, "rt_occluded"))
        o = b["occ"].read()
        assert not (o & ~(h["triangle"] >= 0)).any(), k  # occluded implies hit
        frac[k] = (float((h["triangle"] >= 0).mean()), float(o.mean()))
    times = gpu_timing.interleaved(variants, launch, a.warmup, a.reps)
    records = []
    for k in sets:
        base = np.array(times[(k, "rt_trace_rays")])
        base_spread = float(base.max() - base.min())
        for call in ("rt_trace_rays", "rt_occluded"):
            med = float(np.median(times[(k, call)]))
            rec = {"scene": a.scene, "set": k, "call": call, "rays": bufs[k]["n"], **gpu_timing.summary(times[(k, call)], 4),
                   "mrays_per_s_median": round(bufs[k]["n"] / med / 1e3, 1), "hit_fraction": round(frac[k][0], 4)}
            if call == "rt_occluded":
                rec["occluded_fraction"] = round(frac[k][1], 4)
                rec["speedup_over_trace_rays"] = round(float(np.median(base)) / med, 3)
                rec["not_slower_within_trace_rays_spread"] = bool(med <= float(np.median(base)) + base_spread)
                rec["early_share"] = early[k] if early else None
            records.append(rec)
    gpu_timing.write_lines(a.out, records)


if __name__ == "__main__":
    main()
