"""The path samplers (rt_sample_paths, rt_sampler_rays, rt_sampler_rays_host;
include/isaklm_rt.h, DESIGN.md §11 "Samplers") without a GPU: the host twin
(csrc/host/sampler_host.cpp, the text the kernels compile) against the numpy
restatement tests/sampler_ref.py bit for bit, the pinhole sampler against the
restatement tests/test_paths_cpu.py pins to the oracle, the geometry of every
kind against closed formulas in float64, the hemisphere's distribution, and the
argument checks.

sampler_ref's sine and cosine (independent.sinf / cosf) are the correctly
rounded functions, the library's rt_sincosf (rt_libm.h) may differ from them in
rare hard-to-round cases.  Seeds, cameras and shapes here are fixed, so the
bitwise comparisons below are themselves the check that these inputs hit no
such case: one hit would show as a one-ulp difference in a named ray.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import independent as ind
import oracle
import path_query_ref as pq
import rt
import sampler_ref as sr

f32 = np.float32
E_INVALID = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")

SHAPES = [(1, 1), (3, 2), (67, 45), (96, 54)]
IMAGE = [("pinhole", sr.PINHOLE), ("equirect", sr.EQUIRECT), ("fisheye", sr.FISHEYE), ("ortho", sr.ORTHO)]
# position, yaw, pitch, FOV, aperture (FISHEYE reads FOV as the angle across the image circle)
CAM = np.array([0.3, 1.1, -2.2, 0.4, -0.15, 1.2, 0.03], f32)
ORTHO_HALF = 1.75


def camera(c7):
    c = rt.Camera()
    c.position.x, c.position.y, c.position.z = (float(v) for v in c7[:3])
    c.yaw, c.pitch, c.FOV, c.aperture_radius = (float(v) for v in c7[3:7])
    return c


def sampler(kind, W, H, c7=CAM, pixels=None, half=ORTHO_HALF):
    return rt.Sampler(kind, W, H, camera(c7), ortho_half_width=half, pixels=pixels)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def assert_rays(got, want, what):
    (gr, gs), (wr, ws) = got, want
    assert gr.dtype == f32 and gs.dtype == np.uint32, what
    bad = np.nonzero((gr.view(np.uint32) != wr.view(np.uint32)).any(axis=1))[0]
    assert len(bad) == 0, (what, f"{len(bad)} of {len(gr)} rays differ", bad[:8], gr[bad[:3]], wr[bad[:3]])
    assert np.array_equal(gs, ws), (what, "rng")


def test_header_and_binding():
    text = open(os.path.join(INC, "isaklm_rt.h")).read()
    assert int(re.search(r"#define RT_ABI_VERSION (\d+)", text).group(1)) == 12
    assert rt.ABI_VERSION == 12 and rt.lib().rt_abi_version() == 12
    assert re.search(r"^#define RT_HAS_PATH_SAMPLERS 1$", text, re.M)
    for k, name in enumerate(("PINHOLE", "EQUIRECT", "FISHEYE", "ORTHO", "HEMISPHERE")):
        assert re.search(rf"^#define RT_SAMPLER_{name} {k}$", text, re.M)
        assert getattr(rt, "SAMPLER_" + name) == k
    for fn in ("rt_sample_paths", "rt_sampler_rays", "rt_sampler_rays_host"):
        assert re.search(rf"int {fn}\(", text) and hasattr(rt.lib(), fn)
    assert [n for n, _ in rt.RtSampler._fields_] == ["kind", "width", "height", "camera", "ortho_half_width",
                                                    "pixels_device", "points_device"]


# ---- the host twin against the restatement ----
@pytest.mark.parametrize("name,kind", IMAGE)
@pytest.mark.parametrize("W,H", SHAPES)
def test_host_equals_restatement(name, kind, W, H):
    """three successive samples of the whole frame, the state fed back"""
    st = oracle.mt19937(W * H, skip=7 * kind)
    ref = st.copy()
    smp = sampler(kind, W, H)
    for k in range(3):
        rays, st = rt.sampler_rays_host(smp, st)
        want = sr.image_rays(kind, CAM, W, H, ref, ortho_half_width=ORTHO_HALF)
        assert_rays((rays, st), want, f"{name} {W}x{H} sample {k}")
        ref = want[1]


@pytest.mark.parametrize("name,kind", IMAGE)
def test_host_pixel_list(name, kind):
    """a list with out-of-range and repeated indices: the former give o = d = +0 and leave the state"""
    W, H = 67, 45
    i32 = np.iinfo(np.int32)
    pix = np.array([0, 5, 5, W * H - 1, W * H, -1, i32.min, i32.max, 1234, 5, W * H + 7, 66], np.int32)
    st0 = oracle.mt19937(len(pix), skip=100)
    rays, st = rt.sampler_rays_host(sampler(kind, W, H, pixels=pix), st0)
    assert_rays((rays, st), sr.image_rays(kind, CAM, W, H, st0, pixels=pix, ortho_half_width=ORTHO_HALF), name)
    out = (pix < 0) | (pix >= W * H)
    assert out.sum() == 5
    assert (rays[out].view(np.uint32) == 0).all() and np.array_equal(st[out], st0[out])
    assert (st[~out] != st0[~out]).all()
    # the listed pixel's ray is the frame's ray of that pixel from the same state (repeated pixels: each alone)
    for i in np.nonzero(~out)[0]:
        seeds = np.zeros(W * H, np.uint32)
        seeds[pix[i]] = st0[i]
        fr, fs = rt.sampler_rays_host(sampler(kind, W, H), seeds)
        assert same_bits(fr[pix[i]], rays[i]) and fs[pix[i]] == st[i]


def hemisphere_points(m, seed=3):
    """points with unit normals, the axes and +-z among them"""
    rs = np.random.RandomState(seed)
    n = rs.standard_normal((m, 3))
    n /= np.linalg.norm(n, axis=1)[:, None]
    n = n.astype(f32)
    axes = np.array([[0, 0, 1], [0, 0, -1], [1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [1, 0, -0.0]], f32)
    n[:len(axes)] = axes[:m]
    p = rs.uniform(-3, 3, (m, 3)).astype(f32)
    return np.concatenate([p, n], axis=1)


@pytest.mark.parametrize("m", [1, 6, 3015, 5184])
def test_host_hemisphere_equals_restatement(m):
    pts = hemisphere_points(m)
    st = oracle.mt19937(m, skip=31)
    ref = st.copy()
    smp = rt.Sampler("hemisphere", points=pts)
    for k in range(3):
        rays, st = rt.sampler_rays_host(smp, st)
        want = sr.hemisphere_rays(pts, ref)
        assert_rays((rays, st), want, f"hemisphere {m} sample {k}")
        ref = want[1]
    assert same_bits(rays[:, :3], pts[:, :3])


def test_draw_counts():
    """each kind advances the state by exactly its number of draws"""
    W, H = 3, 2
    st0 = oracle.mt19937(W * H)
    for name, kind in IMAGE:
        want = st0.copy()
        for _ in range(sr.DRAWS[kind]):
            _, want = ind.rng_next(want)
        _, st = rt.sampler_rays_host(sampler(kind, W, H), st0)
        assert np.array_equal(st, want), name
    want = st0.copy()
    for _ in range(2):
        _, want = ind.rng_next(want)
    _, st = rt.sampler_rays_host(rt.Sampler("hemisphere", points=hemisphere_points(W * H)), st0)
    assert np.array_equal(st, want)


# ---- PINHOLE against the restatement that is pinned to the oracle ----
@pytest.mark.parametrize("W,H", [(8, 8), (67, 45), (96, 54), (3, 2)])
@pytest.mark.parametrize("aperture", [0.0, 0.05])
def test_pinhole_is_the_renderers_camera_sample(W, H, aperture):
    cam = CAM.copy()
    cam[6] = aperture
    st = oracle.mt19937(W * H)
    rays, out = rt.sampler_rays_host(sampler("pinhole", W, H, cam), st)
    assert_rays((rays, out), pq.camera_samples(cam, W, H, st), f"pinhole {W}x{H} aperture {aperture}")
    sub = np.array([W * H - 1, 0, 2, 2], np.int32)
    rays, out = rt.sampler_rays_host(sampler("pinhole", W, H, cam, pixels=sub), st[:4])
    assert_rays((rays, out), pq.camera_samples(cam, W, H, st[:4], pixels=sub), "pinhole pixel list")


# ---- centre rays ----
@pytest.mark.parametrize("name,kind", IMAGE)
@pytest.mark.parametrize("W,H", SHAPES)
def test_centre_rays_equal_restatement(name, kind, W, H):
    rays = rt.sampler_rays_host(sampler(kind, W, H))
    want, st = sr.image_rays(kind, CAM, W, H, np.zeros(W * H, np.uint32), ortho_half_width=ORTHO_HALF, centre=True)
    assert same_bits(rays, want), name
    assert (st == 0).all()  # nothing is drawn
    if kind != sr.ORTHO:
        assert same_bits(rays[:, :3], np.broadcast_to(CAM[:3], (W * H, 3)).copy())  # no lens offset


def test_hemisphere_has_no_centre_ray():
    smp = rt.Sampler("hemisphere", points=hemisphere_points(4))
    with pytest.raises(rt.RtError):
        rt.sampler_rays_host(smp)


# ---- geometry, independent of the restatement: closed formulas in float64 ----
def rotation64(yaw, pitch):
    """rows i, j, k of rotation_matrix(yaw, pitch, 0) = Rz(0) * Ry(yaw) * Rx(pitch), columns of the matrix"""
    cy, sy, cp, sp = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch)
    ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    rx = np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
    return ry @ rx


def centre_rays64(kind, c7, W, H, half):
    c = np.asarray(c7, np.float64)
    R = rotation64(c[3], c[4])
    e = np.arange(W * H)
    x, y = (e % W) + 0.5, (e // W) + 0.5
    o = np.broadcast_to(c[:3], (W * H, 3)).copy()
    if kind == sr.PINHOLE:
        t = np.tan(c[5] / 2)
        v = np.stack([t * (x - W // 2) / (W // 2), t * (y - H // 2) / (W // 2), np.ones_like(x)], axis=1)
        v /= np.linalg.norm(v, axis=1)[:, None]
    elif kind == sr.EQUIRECT:
        lon, lat = x / W * 2 * np.pi - np.pi, y / H * np.pi - np.pi / 2
        v = np.stack([np.cos(lat) * np.sin(lon), np.sin(lat), np.cos(lat) * np.cos(lon)], axis=1)
    elif kind == sr.FISHEYE:
        rad = min(W, H) / 2
        u, w = (x - W / 2) / rad, (y - H / 2) / rad
        r = np.hypot(u, w)
        th = r * c[5] / 2
        k = np.where(r > 0, np.sin(th) / np.where(r > 0, r, 1), 0)
        v = np.stack([k * u, k * w, np.cos(th)], axis=1)
        v[r > 1] = 0
    else:
        u, w = (x - W / 2) / (W / 2) * half, (y - H / 2) / (W / 2) * half
        o = o + np.outer(u, R[:, 0]) + np.outer(w, R[:, 1])
        v = np.broadcast_to(np.array([0.0, 0.0, 1.0]), (W * H, 3))
    return np.concatenate([o, v @ R.T], axis=1)


@pytest.mark.parametrize("name,kind", IMAGE)
@pytest.mark.parametrize("W,H", [(3, 2), (67, 45), (96, 54)])
def test_centre_rays_against_closed_formulas(name, kind, W, H):
    """within 1e-5 absolute per component (about 16 float32 roundings of relative 2^-24 on intermediates of at
    most 2 pi: 6e-6): axis and sign errors, not rounding.  The pi here is float64's, the library's the
    reference's 3.1415926536f: 9e-8 apart."""
    rays = rt.sampler_rays_host(sampler(kind, W, H)).astype(np.float64)
    want = centre_rays64(kind, CAM, W, H, ORTHO_HALF)
    if kind == sr.FISHEYE:  # (a pixel centre within rounding of the circle may fall on either side)
        x, y = (np.arange(W * H) % W) + 0.5, (np.arange(W * H) // W) + 0.5
        r = np.hypot(x - W / 2, y - H / 2) / (min(W, H) / 2)
        keep = np.abs(r - 1) > 1e-6
        rays, want = rays[keep], want[keep]
    assert np.abs(rays - want).max() <= 1e-5, (name, np.abs(rays - want).max())


def test_equirect_directions_fall_inside_their_texels():
    W, H = 67, 45
    cam = CAM.copy()
    cam[3:5] = 0  # R = identity: the direction's own longitude and latitude
    st = oracle.mt19937(W * H, skip=5)
    rays, _ = rt.sampler_rays_host(sampler("equirect", W, H, cam), st)
    d = rays[:, 3:].astype(np.float64)
    assert np.abs(np.linalg.norm(d, axis=1) - 1).max() < 1e-6
    lon, lat = np.arctan2(d[:, 0], d[:, 2]), np.arcsin(np.clip(d[:, 1], -1, 1))
    fx, fy = (lon + np.pi) / (2 * np.pi) * W, (lat + np.pi / 2) / np.pi * H
    e = np.arange(W * H)
    eps = 1e-4  # texels: ~6 float32 roundings at |lon| <= pi, 3e-6 rad, times W / 2 pi
    assert ((fx >= (e % W) - eps) & (fx <= (e % W) + 1 + eps)).all()
    assert ((fy >= (e // W) - eps) & (fy <= (e // W) + 1 + eps)).all()
    assert (np.floor(fx) == e % W).mean() > 0.99 and (np.floor(fy) == e // W).mean() > 0.99


def test_fisheye_outside_the_circle():
    W, H = 96, 54
    st0 = oracle.mt19937(W * H, skip=9)
    rays, st = rt.sampler_rays_host(sampler("fisheye", W, H), st0)
    e = np.arange(W * H)
    x, y = e % W, e // W
    # pixels whose every point lies outside / inside the circle of radius H / 2 about (W / 2, H / 2)
    nx, ny = np.clip(W / 2, x, x + 1), np.clip(H / 2, y, y + 1)
    fx, fy = np.where(np.abs(x - W / 2) > np.abs(x + 1 - W / 2), x, x + 1), \
        np.where(np.abs(y - H / 2) > np.abs(y + 1 - H / 2), y, y + 1)
    outside = np.hypot(nx - W / 2, ny - H / 2) > H / 2 + 1e-3
    inside = np.hypot(fx - W / 2, fy - H / 2) < H / 2 - 1e-3
    assert outside.sum() > 1000 and inside.sum() > 1000 and outside[0] and outside[W - 1] and outside[-1]
    assert (rays[outside, 3:].view(np.uint32) == 0).all()
    assert same_bits(rays[outside, :3], np.broadcast_to(CAM[:3], (int(outside.sum()), 3)).copy())
    assert np.abs(np.linalg.norm(rays[inside, 3:].astype(np.float64), axis=1) - 1).max() < 1e-5
    want = st0.copy()
    for _ in range(2):
        _, want = ind.rng_next(want)
    assert np.array_equal(st, want)  # the 2 draws are taken inside and outside alike


def test_ortho_is_a_parallel_grid():
    W, H = 67, 45
    rays = rt.sampler_rays_host(sampler("ortho", W, H)).astype(np.float64)
    d, o = rays[:, 3:], rays[:, :3].reshape(H, W, 3)
    assert (rays[:, 3:] == rays[0, 3:]).all()
    assert np.abs(np.linalg.norm(d[0]) - 1) < 1e-6
    assert np.abs((o - o[0, 0]) @ d[0]).max() < 1e-5  # coplanar, the plane normal to the direction
    step = 2 * ORTHO_HALF / W
    assert np.abs(np.linalg.norm(o[:, 1:] - o[:, :-1], axis=2) - step).max() < 1e-5
    assert np.abs(np.linalg.norm(o[1:] - o[:-1], axis=2) - step).max() < 1e-5  # square pixels
    assert abs((o[0, 1] - o[0, 0]) @ (o[1, 0] - o[0, 0])) < 1e-5  # rows at right angles to columns


def test_hemisphere_distribution():
    """65,536 samples about unit normals (the axes and +-z among them)"""
    m = 65536
    pts = hemisphere_points(m)
    n = pts[:, 3:].astype(np.float64)
    rays, _ = rt.sampler_rays_host(rt.Sampler("hemisphere", points=pts), oracle.mt19937(m, skip=77))
    d = rays[:, 3:].astype(np.float64)
    cos = np.einsum("ij,ij->i", d, n)
    assert cos.min() >= -1e-6
    # cosine-weighted: the mean of cos is 2/3, its standard deviation 0.236: 0.005 is 5 standard errors
    assert abs(cos.mean() - 2 / 3) <= 0.005, cos.mean()
    assert np.abs(np.linalg.norm(d, axis=1) - 1).max() <= 1e-5
    # one normal, many states: the same three properties (here for -z, the frame's other sheet)
    for normal in ([0, 0, -1], [0, 0, 1], [1, 0, 0]):
        one = np.tile(np.array([0, 0, 0] + normal, f32), (m, 1))
        rays, _ = rt.sampler_rays_host(rt.Sampler("hemisphere", points=one), oracle.mt19937(m))
        d = rays[:, 3:].astype(np.float64)
        cos = d @ np.array(normal, np.float64)
        assert cos.min() >= -1e-6 and abs(cos.mean() - 2 / 3) <= 0.005, (normal, cos.mean())
        assert np.abs(np.linalg.norm(d, axis=1) - 1).max() <= 1e-5


# ---- argument errors ----
def test_argument_errors_without_a_device():
    """Every rejected call returns RT_E_INVALID before it looks at the scene or the device: the scene handle is
    not a scene and the pointers are not device memory."""
    L = rt.lib()
    fake, good = 0x1000, 0x2000
    W, H = 4, 3
    n = W * H

    def smp(kind=rt.SAMPLER_PINHOLE, width=W, height=H, fov=1.0, half=1.0, pixels=None, points=None, **cam):
        c = camera(CAM)
        c.FOV = fov
        for k, v in cam.items():
            setattr(c, k, v)
        return rt.RtSampler(kind, width, height, c, half, pixels, points)

    def sample(s, scene=fake, rng=good, n=n, rad=good, sq=good, cnt=good, opt=None):
        return L.rt_sample_paths(scene, ctypes.byref(s) if s is not None else None, rng, n, rad, sq, cnt, opt)

    def rays_dev(s, rng=good, n=n, rays=good):
        return L.rt_sampler_rays(ctypes.byref(s) if s is not None else None, rng, n, rays, None)

    def rays_host(s, rng=good, n=n, rays=good):
        return L.rt_sampler_rays_host(ctypes.byref(s) if s is not None else None, rng, n, rays)

    inf, nan = float("inf"), float("nan")
    bad_samplers = [
        (None, "null sampler"),
        (smp(kind=-1), "kind -1"),
        (smp(kind=5), "kind 5"),
        (smp(width=0), "width 0"),
        (smp(height=0), "height 0"),
        (smp(width=-3), "width < 0"),
        (smp(width=1 << 16, height=1 << 15), "width * height = 2^31"),
        (smp(width=W + 1), "no pixel list and n != width * height"),
        (smp(pixels=good + 2), "misaligned pixel list"),
        (smp(kind=rt.SAMPLER_FISHEYE, fov=0.0), "fisheye FOV 0"),
        (smp(kind=rt.SAMPLER_FISHEYE, fov=-1.0), "fisheye FOV < 0"),
        (smp(kind=rt.SAMPLER_FISHEYE, fov=6.3), "fisheye FOV > 2 pi"),
        (smp(kind=rt.SAMPLER_FISHEYE, fov=inf), "fisheye FOV inf"),
        (smp(kind=rt.SAMPLER_FISHEYE, fov=nan), "fisheye FOV NaN"),
        (smp(kind=rt.SAMPLER_ORTHO, half=0.0), "ortho half width 0"),
        (smp(kind=rt.SAMPLER_ORTHO, half=-2.0), "ortho half width < 0"),
        (smp(kind=rt.SAMPLER_ORTHO, half=inf), "ortho half width inf"),
        (smp(kind=rt.SAMPLER_ORTHO, half=nan), "ortho half width NaN"),
        (smp(kind=rt.SAMPLER_HEMISPHERE), "hemisphere without points"),
        (smp(kind=rt.SAMPLER_HEMISPHERE, points=good + 4), "hemisphere points not 8-B aligned"),
    ]
    for s, what in bad_samplers:
        for call in (sample, rays_dev, rays_host):
            assert call(s) == E_INVALID, (what, call.__name__)
            assert L.rt_last_error(), what
    ok = smp()
    # what rt_trace_paths checks
    for change, what in ((dict(scene=None), "null scene"), (dict(rng=None), "null rng"), (dict(rad=None), "null radiance"),
                         (dict(n=-1), "n < 0"), (dict(n=1 << 31), "n > 2^31 - 1"), (dict(rng=good + 2), "rng misaligned"),
                         (dict(rad=good + 1), "radiance misaligned"), (dict(sq=good + 3), "sq misaligned"),
                         (dict(cnt=good + 2), "sample_count misaligned")):
        assert sample(ok, **change) == E_INVALID, what
    for bad, what in ((dict(samples=-1), "samples < 0"), (dict(samples=(1 << 20) + 1), "samples > 2^20"),
                      (dict(max_depth=-1), "max_depth < 0"), (dict(max_depth=1 << 24), "max_depth > 2^24 - 1"),
                      (dict(accumulate=2), "accumulate 2"), (dict(traversal=77), "traversal"),
                      (dict(stats=good + 4), "stats not 8-B aligned")):
        assert sample(ok, opt=ctypes.byref(rt.path_options(**bad))) == E_INVALID, what
    for call in (rays_dev, rays_host):
        assert call(ok, rays=None) == E_INVALID
        assert call(ok, n=-1) == E_INVALID
        assert call(smp(kind=rt.SAMPLER_HEMISPHERE, points=good), rng=None) == E_INVALID  # no centre ray
    assert rays_dev(ok, rays=good + 4) == E_INVALID and rays_dev(ok, rng=good + 2) == E_INVALID
    # the valid ranges' ends are accepted; n == 0: RT_OK, no launch, nothing is looked at
    listed = smp(pixels=good)
    assert sample(listed, n=0) == 0 and sample(listed, n=0, sq=None, cnt=None) == 0
    assert rays_dev(listed, n=0) == 0 and rays_host(listed, n=0) == 0
    assert sample(smp(kind=rt.SAMPLER_HEMISPHERE, points=good), n=0) == 0
    assert sample(smp(kind=rt.SAMPLER_FISHEYE, fov=float(ind.TAU), pixels=good), n=0) == 0
    assert sample(smp(kind=rt.SAMPLER_ORTHO, half=1e-30, pixels=good), n=0) == 0
    assert sample(smp(width=1, height=1, pixels=good), n=0) == 0
    # NaN and infinite camera fields are no error
    assert sample(smp(yaw=nan, pitch=inf, fov=nan, aperture_radius=inf, pixels=good), n=0) == 0


def test_binding_argument_errors():
    smp = sampler("pinhole", 4, 3)
    for bad_call in (lambda: rt.sampler_rays_host(smp, np.zeros(11, np.uint32)),
                     lambda: rt.sampler_rays_host(smp, np.zeros(12, np.int32)),
                     lambda: rt.sample_paths(None, smp, np.zeros(11, np.uint32)),
                     lambda: rt.sample_paths(None, smp, np.zeros(12, np.uint32), sq=np.zeros(12, f32)),
                     lambda: rt.sample_paths(None, smp, np.zeros(12, np.uint32), radiance=np.zeros((12, 3), np.float64)),
                     lambda: rt.sample_paths(None, smp, np.zeros(12, np.uint32), count=np.zeros(12, np.int32)),
                     lambda: rt.Sampler("hemisphere", points=np.zeros((4, 5), f32))):
        with pytest.raises(ValueError):
            bad_call()
    with pytest.raises(KeyError):
        rt.Sampler("cylindrical")
