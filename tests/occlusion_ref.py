"""The occlusion tests' reference for a hit's ray parameter s, and the
host checker (tests/native/occlusion_check.cpp) — shared by
tests/test_occlusion_cpu.py and tests/test_gpu_occlusion.py.

s is the *t of the reference's winning intersect_triangle
(rt/trace_ray.cuh:75-90), restated here in float32 numpy on the hit triangle
the oracle names — never taken from the code under test:

    normal = normalize(cross(p2 - p1, p3 - p1))
    s = (dot(normal, p1) - dot(ray.position, normal)) / dot(ray.direction, normal)

test_occlusion_cpu.py pins it, bit for bit, to the checker's own plain-KD
restatement on the very ray sets the GPU tests use.
"""
import os
import subprocess

import numpy as np

import helpers
import independent as ind

f32 = np.float32
THRESHOLD_KINDS = ("inbox", "outside", "gate:4")  # the ray sets of the bit-exact threshold tests


def s_reference(tris, rays, tri):
    """s of ray i on triangle tri[i] (entries with tri < 0 are computed on triangle 0 and mean nothing);
    tris: the reference-layout triangles, (n, 152) uint8 (p1, p2, p3 first)"""
    rays = np.ascontiguousarray(rays, dtype=f32)
    p = tris[:, :36].copy().view(f32).reshape(-1, 3, 3)[np.maximum(np.asarray(tri, np.int64), 0)]
    p1, p2, p3 = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        normal = ind.normalize(ind.cross(p2 - p1, p3 - p1))
        dn = ind.dot(rays[:, 3:], normal)
        d = ind.dot(normal, p1)
        s = (d - ind.dot(rays[:, :3], normal)) / dn
    assert s.dtype == f32
    return s


def build_checker(outdir):
    """compiles tests/native/occlusion_check.cpp against the built library; returns the binary's path"""
    return helpers.build_native(outdir, "occlusion_check", openmp=False)


DUMP = np.dtype([("hit", "<i4"), ("triangle", "<i4"), ("s", "<f4")])


def checker_dump(checker, scene, rays, workdir):
    """the checker's plain-KD restatement of trace_ray on `rays`: a DUMP record per ray"""
    f, o = os.path.join(str(workdir), "rays.f32"), os.path.join(str(workdir), "dump.bin")
    np.ascontiguousarray(rays, dtype=f32).tofile(f)
    r = subprocess.run([checker, scene, "dump", f, o], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return np.fromfile(o, dtype=DUMP)
