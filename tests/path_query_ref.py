"""The mapping from a frame's camera samples to a ray list (TEST
INFRASTRUCTURE ONLY): what rt_trace_paths (include/isaklm_rt.h) is compared
through with the oracle's or_render.

camera_samples restates the sample set-up of independent_path.render (the
lines between `st = int(rng[i])` and the trace_path call: two jitter draws,
the direction through rotation_matrix, the two pinhole draws, the origin) on
numpy float32 arrays, operation for operation.  By construction: if `seeds` is
a frame's RNG and (rays, st) this function's output, one or_render pass from
reset leaves fb = +0 + trace_path(rays, st).L, sq = luminance(L)^2 and rng =
the state after the path.  tests/test_paths_cpu.py pins it to the scalar code
and to the oracle.
"""
import numpy as np

import independent as ind
import independent_path as ip

f32 = np.float32


def _mat_vec(R, x, y, z):
    """independent_path.mat_vec on component arrays: (x * i + y * j) + z * k, as an (m, 3) array"""
    return np.stack([(x * R[0][a] + y * R[1][a]) + z * R[2][a] for a in range(3)], axis=1).astype(f32)


def camera_samples(camera7, W, H, seeds, pixels=None):
    """-> (rays (m, 6) float32, rng_after (m,) uint32) for the pixels `pixels` (indices y * W + x; None: all, in
    order) of a W x H frame of camera (x, y, z, yaw, pitch, fov, aperture) whose RNG states are `seeds` (one per
    listed pixel): each pixel's next camera sample and its RNG state after the four set-up draws."""
    cam = np.asarray(camera7, f32)
    pos = cam[:3]
    yaw, pitch, fov, aperture = (f32(x) for x in cam[3:7])
    R = ip.rotation_matrix(yaw, pitch)
    tan_half = f32(np.tan(np.float64(fov / f32(2))))
    hw, hh = f32(W // 2), f32(H // 2)
    px = np.arange(W * H) if pixels is None else np.asarray(pixels, np.int64)
    st = np.ascontiguousarray(seeds, np.uint32)
    assert st.shape == px.shape
    x, y = (px % W).astype(f32), (px // W).astype(f32)
    rx, st = ind.rng_next(st)
    ry, st = ind.rng_next(st)
    dx = tan_half * ((x + rx) - hw) / hw
    dy = tan_half * ((y + ry) - hh) / hw
    one = np.ones_like(dx)
    r = f32(1) / np.sqrt(dx * dx + dy * dy + one * one)
    d = _mat_vec(R, dx * r, dy * r, one * r)
    th, st = ind.rng_next(st)
    theta = th * ind.TAU
    rr, st = ind.rng_next(st)
    rad = np.sqrt(rr) * aperture
    ox = rad * ind.cosf(theta)
    oy = rad * ind.sinf(theta)
    zero = np.zeros_like(ox)
    o = (pos[None, :] + _mat_vec(R, ox, zero, zero)) + _mat_vec(R, zero, oy, zero)
    rays = np.concatenate([o, d], axis=1).astype(f32)
    assert rays.dtype == f32 and dx.dtype == f32 and theta.dtype == f32 and rad.dtype == f32
    return rays, st


def scalar_paths(scene, rays, rng, samples=1):
    """independent_path.Scene.trace_path on each ray, `samples` times, summed in sample order from +0:
    -> (radiance (m, 3), sq (m,), rng_after (m,))"""
    m = len(rays)
    rad, sq, out = np.zeros((m, 3), f32), np.zeros(m, f32), np.zeros(m, np.uint32)
    for i in range(m):
        o, d = tuple(f32(v) for v in rays[i, :3]), tuple(f32(v) for v in rays[i, 3:])
        st = int(rng[i])
        acc, s2 = ip.v(0, 0, 0), f32(0)
        for _ in range(samples):
            with np.errstate(all="ignore"):
                L, st = scene.trace_path(o, d, st)
                acc = ip.add(acc, L)
                lum = ip.luminance(L)
                s2 = s2 + lum * lum
        rad[i], sq[i], out[i] = acc, s2, st
    return rad, sq, out


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32) if np.asarray(a).dtype == f32 else np.asarray(a)


def assert_same(got, want, what):
    """(radiance, sq, rng) triples, bit for bit"""
    for name, a, b in zip(("radiance", "sq", "rng"), got, want):
        a, b = np.asarray(a), np.asarray(b).reshape(np.asarray(a).shape)
        assert a.dtype == b.dtype, (what, name, a.dtype, b.dtype)
        differ = bits(a) != bits(b)
        bad = np.nonzero(differ.any(axis=1) if differ.ndim == 2 else differ)[0]
        assert len(bad) == 0, (what, name, f"{len(bad)} of {len(a)} rays differ", bad[:8], a[bad[:3]], b[bad[:3]])
