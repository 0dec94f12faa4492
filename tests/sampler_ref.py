"""The ray samplers of rt_sample_paths / rt_sampler_rays (include/isaklm_rt.h,
DESIGN.md §11 "Samplers") restated in numpy float32, operation for operation
(TEST INFRASTRUCTURE ONLY).  Built on tests/independent.py (rng_next, the
correctly rounded sinf / cosf, TAU) and independent_path.rotation_matrix;
nothing of the library is used.
"""
import numpy as np

import independent as ind
import independent_path as ip

f32 = np.float32
PINHOLE, EQUIRECT, FISHEYE, ORTHO, HEMISPHERE = range(5)
IMAGE_KINDS = (PINHOLE, EQUIRECT, FISHEYE, ORTHO)
DRAWS = {PINHOLE: 4, EQUIRECT: 2, FISHEYE: 2, ORTHO: 2, HEMISPHERE: 2}
HALF = f32(0.5)


def _mat_vec(R, x, y, z):
    """R * v = (x * i + y * j) + z * k on component arrays -> (m, 3)"""
    return np.stack([(x * R[0][a] + y * R[1][a]) + z * R[2][a] for a in range(3)], axis=1).astype(f32)


def _draw(st, centre):
    if centre:
        return np.full(st.shape, HALF, f32), st
    return ind.rng_next(st)


def image_rays(kind, camera7, W, H, seeds, pixels=None, ortho_half_width=1.0, centre=False):
    """-> (rays (m, 6) float32, rng_after (m,) uint32): one sample of an image sampler of camera (x, y, z, yaw,
    pitch, fov, aperture) for the listed pixels (None: all).  centre: both jitter draws 0.5, no lens, no draw."""
    cam = np.asarray(camera7, f32)
    pos = cam[:3]
    yaw, pitch, fov, aperture = (f32(v) for v in cam[3:7])
    R = ip.rotation_matrix(yaw, pitch)
    px = np.arange(W * H, dtype=np.int64) if pixels is None else np.asarray(pixels, np.int32).astype(np.int64)
    seeds = np.ascontiguousarray(seeds, np.uint32)
    assert seeds.shape == px.shape
    m = len(px)
    rays = np.zeros((m, 6), f32)
    out = seeds.copy()
    ok = ((px & 0xFFFFFFFF) < W * H)  # compared unsigned
    if not ok.any():
        return rays, out
    p, st = px[ok], seeds[ok]
    x, y = (p % W).astype(f32), (p // W).astype(f32)
    Wf, Hf = f32(W), f32(H)
    with np.errstate(all="ignore"):
        rx, st = _draw(st, centre)
        ry, st = _draw(st, centre)
        zero = np.zeros_like(rx)
        one = np.ones_like(rx)
        posn = np.broadcast_to(pos[None, :], (len(p), 3)).astype(f32)
        if kind == PINHOLE:
            tan_half = f32(np.tan(np.float64(fov / f32(2))))
            hw, hh = f32(W // 2), f32(H // 2)
            dx = tan_half * ((x + rx) - hw) / hw
            dy = tan_half * ((y + ry) - hh) / hw
            r = f32(1) / np.sqrt(dx * dx + dy * dy + one * one)
            d = _mat_vec(R, dx * r, dy * r, one * r)
            o = posn
            if not centre:
                th, st = ind.rng_next(st)
                theta = th * ind.TAU
                rr, st = ind.rng_next(st)
                rad = np.sqrt(rr) * aperture
                ox = rad * ind.cosf(theta)
                oy = rad * ind.sinf(theta)
                o = (posn + _mat_vec(R, ox, zero, zero)) + _mat_vec(R, zero, oy, zero)
        elif kind == EQUIRECT:
            lon = (x + rx) / Wf * ind.TAU - ind.PI
            lat = (y + ry) / Hf * ind.PI - ind.PI * HALF
            sl, cl = ind.sinf(lon), ind.cosf(lon)
            sa, ca = ind.sinf(lat), ind.cosf(lat)
            d = _mat_vec(R, ca * sl, sa, ca * cl)
            o = posn
        elif kind == FISHEYE:
            rad = f32(min(W, H)) * HALF
            u = ((x + rx) - Wf * HALF) / rad
            v = ((y + ry) - Hf * HALF) / rad
            r = np.sqrt(u * u + v * v)
            inside = r <= f32(1)
            theta = r * (fov * HALF)
            s, c = ind.sinf(theta), ind.cosf(theta)
            k = np.where(r > f32(0), s / np.where(r > f32(0), r, f32(1)), f32(0)).astype(f32)
            d = _mat_vec(R, k * u, k * v, c)
            d[~inside] = 0
            o = posn
        elif kind == ORTHO:
            hwid = f32(ortho_half_width)
            u = ((x + rx) - Wf * HALF) / (Wf * HALF) * hwid
            v = ((y + ry) - Hf * HALF) / (Wf * HALF) * hwid
            o = (posn + _mat_vec(R, u, zero, zero)) + _mat_vec(R, zero, v, zero)
            d = _mat_vec(R, zero, zero, one)
        else:
            raise ValueError(kind)
    rays[ok] = np.concatenate([o, d], axis=1).astype(f32)
    out[ok] = st
    return rays, out


def frame(n):
    """the branch-free orthonormal frame of the (m, 3) normals (Duff et al. 2017) -> t, b"""
    nx, ny, nz = n[:, 0], n[:, 1], n[:, 2]
    with np.errstate(all="ignore"):
        sg = np.copysign(f32(1), nz).astype(f32)
        a = f32(-1) / (sg + nz)
        q = nx * ny * a
        t = np.stack([f32(1) + sg * nx * nx * a, sg * q, -sg * nx], axis=1).astype(f32)
        b = np.stack([q, sg + ny * ny * a, -ny], axis=1).astype(f32)
    return t, b


def hemisphere_rays(points, seeds):
    """-> (rays, rng_after): one cosine-weighted direction about each of the (m, 6) points' normals"""
    pts = np.ascontiguousarray(points, f32)
    st = np.ascontiguousarray(seeds, np.uint32)
    p, n = pts[:, :3], pts[:, 3:]
    with np.errstate(all="ignore"):
        xi, st = ind.rng_next(st)
        phi = xi * ind.TAU
        ds, dc = ind.sinf(phi), ind.cosf(phi)
        ru2, st = ind.rng_next(st)
        sq = np.sqrt(ru2)
        t, b = frame(n)
        d = ((sq * dc)[:, None] * t + np.sqrt(f32(1) - ru2)[:, None] * n) + (sq * ds)[:, None] * b
    assert d.dtype == f32 and phi.dtype == f32
    return np.concatenate([p, d], axis=1).astype(f32), st


def rays(kind, seeds, camera7=None, W=0, H=0, pixels=None, ortho_half_width=1.0, points=None, centre=False):
    if kind == HEMISPHERE:
        return hemisphere_rays(points, seeds)
    return image_rays(kind, camera7, W, H, seeds, pixels, ortho_half_width, centre)
