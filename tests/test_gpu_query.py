"""The batched ray query and the first-hit AOVs on the GPU (rt_trace_rays,
rt_camera_rays, rt_render_aov; csrc/query.hip) against the oracle's
or_trace_rays — the reference's trace_ray — bit for bit, for rays of every
kind a caller may send: unit directions, origins outside the scene, tiny and
huge directions (where the conservative-BVH bound is not proven and the
kernel's domain gate must fall back to the plain KD traversal), rays in a KD
split plane, axis-parallel and non-finite rays.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import hazards
import helpers
import oracle
import rt

pytestmark = pytest.mark.gpu
f32 = np.float32
MODES = [rt.TRAVERSAL_BOUNDED, rt.TRAVERSAL_KD]
N = 4096
SCALES = {"2^-80": 2.0 ** -80, "2^-58": 2.0 ** -58, "1e-3": 1e-3, "7": 7.0, "2^20": 2.0 ** 20, "2^70": 2.0 ** 70}
GATE_SCALES = {"2^-80": 2.0 ** -80, "0.25": 0.25, "0.5": 0.5, "1": 1.0, "2": 2.0, "4": 4.0}


def bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


# ------------------------------------------------------------------ scenes
class _Case:
    """one scene on the device and in the oracle; oracle results are computed once per ray set and shared"""

    def __init__(self, path):
        self.run = helpers.GpuRun(path)
        self.osc = oracle.OracleScene(self.run.path)
        arr = self.osc.arrays()
        self.tris = np.frombuffer(arr[0], np.uint8).reshape(-1, 152)
        self.bounds = arr[4].astype(f32)
        self._sets, self._refs = {}, {}

    def rays(self, kind):
        if kind not in self._sets:
            self._sets[kind] = make_rays(self, kind)
            self._sets[kind].setflags(write=False)
        return self._sets[kind]

    def ref(self, kind):
        if kind not in self._refs:
            self._refs[kind] = self.osc.trace_rays(self.rays(kind))
            self._refs[kind].setflags(write=False)
        return self._refs[kind]


_cases = {}


def case(name):
    if name not in _cases:
        _cases[name] = _Case(name)
    return _cases[name]


def _unit(g, n):
    v = g.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1)[:, None]).astype(f32)


def _inbox(g, c, n):
    return g.uniform(c.bounds[:3], c.bounds[3:], (n, 3)).astype(f32)


def make_rays(c, kind, n=N):
    """the seeded ray sets, (n, 6) float32"""
    if kind == "inbox":
        g = np.random.default_rng(11)
        return np.concatenate([_inbox(g, c, n), _unit(g, n)], axis=1)
    if kind.startswith("scaled:"):  # the in-box unit set, directions scaled (not normalised by anyone)
        r = c.rays("inbox").copy()
        r[:, 3:] = (r[:, 3:].astype(np.float64) * SCALES[kind[7:]]).astype(f32)
        return r
    if kind.startswith("gate:"):  # the same, scales around the gate's edges (powers of two: exact)
        r = c.rays("inbox").copy()
        r[:, 3:] = r[:, 3:] * f32(GATE_SCALES[kind[5:]])
        return r
    g = np.random.default_rng({"outside": 12, "split": 13, "axis": 14, "special": 15}[kind])
    lo, hi = c.bounds[:3].astype(np.float64), c.bounds[3:].astype(np.float64)
    size = hi - lo
    if kind == "outside":  # origins up to 2 box sizes outside the box, aimed loosely at it
        o = g.uniform(lo - 2 * size, hi + 2 * size, (n, 3))
        inside = np.all((o >= lo) & (o <= hi), axis=1)
        o[inside, 0] = lo[0] - size[0] * g.uniform(0.01, 2.0, inside.sum())
        target = g.uniform(lo - 0.5 * size, hi + 0.5 * size, (n, 3))
        d = target - o
        d /= np.linalg.norm(d, axis=1)[:, None]
        return np.concatenate([o, d], axis=1).astype(f32)
    if kind == "split":  # origins on the KD root split plane, the direction lying in it
        axis, off = hazards.root_split(c.osc)
        o, d = _inbox(g, c, n), _unit(g, n)
        o[:, axis] = off
        d[:, axis] = 0.0
        return np.concatenate([o, d], axis=1)
    if kind == "axis":  # axis-parallel: two zero components (of either sign)
        o = _inbox(g, c, n)
        d = np.zeros((n, 3), f32)
        d[np.arange(n), g.integers(0, 3, n)] = g.choice(np.array([-1.0, 1.0, 0.5, -2.0, 1e-3, -3e4], f32), n)
        d[g.random(n) < 0.3] *= f32(-1.0)  # (zeros of both signs)
        return np.concatenate([o, d], axis=1)
    if kind == "special":  # a 64-ray block of non-finite, zero and huge values
        o, d = _inbox(g, c, 64), _unit(g, 64)
        nan, inf = f32(np.nan), f32(np.inf)
        for k in range(0, 12):
            d[k, k % 3] = nan if k < 6 else (inf if k < 9 else -inf)
        d[12:16] = [nan, nan, nan]
        d[16:20] = [inf, -inf, inf]
        d[20:28] = 0.0
        d[28:36] = [0.0, 0.0, -0.0]
        d[36:40] = [-0.0, -0.0, -0.0]
        o[40:48] = f32(3e38) * np.sign(_unit(g, 8))
        o[48:52, 0] = f32(3e38)
        o[52:54] = nan
        o[54:56, 1] = inf
        d[56:60] *= f32(3e38)
        d[60:64] = d[60:64] * f32(1e-30) * f32(1e-15)  # denormals
        return np.concatenate([o, d], axis=1).astype(f32)
    raise KeyError(kind)


def assert_matches_oracle(hits, surf, ref, what):
    """hit flag, triangle, position, normal and tangent: trace_ray's, bit for bit"""
    hit = hits["triangle"] >= 0
    assert np.array_equal(hit, ref[:, 0] == 1), (what, "hit flag", np.nonzero(hit != (ref[:, 0] == 1))[0][:8])
    bad = np.nonzero(hits["triangle"] != ref[:, 1].astype(np.int64))[0]
    assert len(bad) == 0, (what, "triangle", len(bad), bad[:8], hits["triangle"][bad[:8]], ref[bad[:8], 1])
    if surf is not None:
        for name, cols in (("position", slice(2, 5)), ("normal", slice(5, 8)), ("tangent", slice(8, 11))):
            bad = np.nonzero((bits(surf[name]) != bits(ref[:, cols])).any(axis=1))[0]
            assert len(bad) == 0, (what, name, len(bad), bad[:8], surf[name][bad[:3]], ref[bad[:3], cols])
    miss = ~hit
    assert not bits(np.stack([hits["bx"], hits["by"], hits["bz"]], 1))[miss].any(), (what, "miss barycentrics")


# ------------------------------------------------------------------ 1. ray classes
CLASSES = ["inbox", "outside", "split", "axis", "special"] + ["scaled:" + k for k in SCALES]


@pytest.mark.parametrize("kind", CLASSES)
@pytest.mark.parametrize("name", ["cornell", "room_small"])
def test_ray_classes_match_the_oracle(name, kind):
    c = case(name)
    rays, ref = c.rays(kind), c.ref(kind)
    frac = float((ref[:, 0] == 1).mean())
    print(f"{name} {kind}: oracle hits {frac:.3f}")
    # the inputs are not trivial: a test cannot pass by missing (or hitting) everything
    if kind == "inbox":
        assert 0.25 <= frac <= 0.98, frac
    if kind == "outside":
        assert frac >= 0.01, frac
    for mode in MODES:
        hits, surf = rt.trace_rays(c.run.dev, rays, surface=True, traversal=mode)
        assert_matches_oracle(hits, surf, ref, f"{name} {kind} mode {mode}")


# ------------------------------------------------------------------ 2. gate accounting
@pytest.mark.parametrize("scale", list(GATE_SCALES))
@pytest.mark.parametrize("name", ["cornell", "room_small"])
def test_gate_accounting(name, scale):
    """stats[2], the rays the bounded mode hands to the plain KD traversal, is
    exactly the number of rays with max|d_i| outside [0.5, 2]"""
    c = case(name)
    kind = "gate:" + scale
    rays, ref = c.rays(kind), c.ref(kind)
    d = np.abs(rays[:, 3:])
    assert (d != 0).all() and np.isfinite(rays).all()  # so rt_bounded_ray admits every one of them
    m = d.max(axis=1)
    outside = int(((m < f32(0.5)) | (m > f32(2.0))).sum())
    if scale in ("1", "2"):
        assert outside == 0  # unit directions always pass: 1/sqrt(3) <= max|d_i| <= 1
    if scale in ("2^-80", "0.25", "4"):
        assert outside == N
    nhits = int((ref[:, 0] == 1).sum())
    hits, st = rt.trace_rays(c.run.dev, rays, traversal=rt.TRAVERSAL_BOUNDED, stats=True)
    print(f"{name} scale {scale}: outside the gate {outside}, stats {st}")
    assert_matches_oracle(hits, None, ref, kind)
    assert st == {"rays": N, "hits": nhits, "kd_rays": outside}, (st, outside, nhits)
    hits, st = rt.trace_rays(c.run.dev, rays, traversal=rt.TRAVERSAL_KD, stats=True)
    assert st == {"rays": N, "hits": nhits, "kd_rays": N}, st


# ------------------------------------------------------------------ 3. shapes
Dev = rt.DeviceArray  # (the other GPU tests' device buffers too)


def test_device_array():
    """rt.DeviceArray: a round trip of an array and of an empty one, zero(), free() twice, the context manager"""
    a = np.arange(15, dtype=f32).reshape(5, 3)
    d = rt.DeviceArray(a)
    assert d.shape == (5, 3) and d.dtype == f32 and d.p.value
    got = d.read()
    assert got is not a and got.dtype == f32 and np.array_equal(got, a)
    d.upload(a[::-1])
    assert np.array_equal(d.read(), a[::-1])
    d.zero()
    assert d.read().shape == (5, 3) and not d.read().any()
    d.free()
    d.free()
    assert not d.p
    empty = rt.DeviceArray(np.zeros((0, 6), f32))
    assert empty.p.value and empty.read().shape == (0, 6) and empty.read().dtype == f32
    empty.zero()
    empty.free()
    with rt.DeviceArray(7, np.int32, zero=True) as z:
        p = z.p.value
        assert p and z.read().tolist() == [0] * 7
        view = rt.DeviceArray.at(p + 8, (2,), np.int32)
        view.upload([5, 6])
        view.free()  # (not its memory)
        assert z.read().tolist() == [0, 0, 5, 6, 0, 0, 0]
    assert not z.p
    with pytest.raises(ZeroDivisionError):
        with rt.DeviceArray(3, np.uint8) as z:
            1 / 0
    assert not z.p


def _guarded(dtype, n):
    """n records + 64 guard records, every byte 0xCD"""
    return np.frombuffer(bytes([0xCD]) * ((n + 64) * dtype.itemsize), dtype=dtype).copy()


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 257, 300_000])
def test_shapes_and_untouched_tail(n):
    """every n around the wave and block sizes, and more rays than the resident
    grid has threads (the refill loop runs several rounds); the 64 records after
    the n-th keep their 0xCD bytes"""
    c = case("cornell")
    g = np.random.default_rng(100 + n % 97)
    rays = np.concatenate([_inbox(g, c, n), _unit(g, n)], axis=1).astype(f32).reshape(n, 6)
    ref = c.osc.trace_rays(rays) if n else np.zeros((0, 12), f32)
    for mode in MODES:
        d_rays, d_hits, d_surf = Dev(rays), Dev(_guarded(rt.RAY_HIT, n)), Dev(_guarded(rt.RAY_SURFACE, n))
        d_stats = Dev(np.zeros(3, np.uint64))
        try:
            rt.trace_rays_device(c.run.dev, d_rays.p, n, d_hits.p, d_surf.p, traversal=mode, stats_ptr=d_stats.p)
            hits, surf, stats = d_hits.read(), d_surf.read(), d_stats.read()
        finally:
            for d in (d_rays, d_hits, d_surf, d_stats):
                d.free()
        assert (hits[n:].view(np.uint8) == 0xCD).all() and (surf[n:].view(np.uint8) == 0xCD).all(), "tail written"
        assert_matches_oracle(hits[:n], surf[:n], ref, f"n = {n} mode {mode}")
        # the counts of partly filled waves too (unit directions from inside the box: all inside the gate)
        assert list(stats) == [n, int((ref[:, 0] == 1).sum()), n if mode == rt.TRAVERSAL_KD else 0], (n, stats)
        if n >= 255:
            assert 0.25 * n < int((hits["triangle"][:n] >= 0).sum()) < n


# ------------------------------------------------------------------ 4. surface
def test_surface_fields_cornell():
    c = case("cornell")
    rays, ref = c.rays("inbox"), c.ref("inbox")
    hits, surf = rt.trace_rays(c.run.dev, rays, surface=True)
    hit = hits["triangle"] >= 0
    assert 0.25 * N < hit.sum() < N
    # t = magnitude(position - origin) as rt_vecmath.h rounds it: sqrt((dx*dx + dy*dy) + dz*dz), one float32
    # operation at a time (IEEE-exact in numpy as on the device)
    dx, dy, dz = ((surf["position"][:, k] - rays[:, k]).astype(f32) for k in range(3))
    t = np.sqrt(((dx * dx).astype(f32) + (dy * dy).astype(f32)).astype(f32) + (dz * dz).astype(f32)).astype(f32)
    assert np.array_equal(bits(surf["t"][hit]), bits(t[hit]))
    # the Cornell box is untextured: a hit's albedo and emittance are its material's (Triangle.material at
    # byte 96: albedo, emittance)
    tri = hits["triangle"][hit]
    assert np.array_equal(bits(surf["albedo"][hit]), c.tris[tri, 96:108].copy().view(np.uint32))
    assert np.array_equal(bits(surf["emittance"][hit]), c.tris[tri, 108:120].copy().view(np.uint32))
    assert (surf["emittance"][hit] > 0).any() and (surf["emittance"][hit] == 0).any()  # lamp and walls
    # misses: zeros, t = +inf
    miss = ~hit
    assert np.all(np.isposinf(surf["t"][miss]))
    for name in ("position", "normal", "tangent", "albedo", "emittance"):
        assert not bits(surf[name][miss]).any(), name
    # the normal faces the ray
    assert np.all(np.einsum("ij,ij->i", surf["normal"][hit].astype(np.float64), rays[hit, 3:].astype(np.float64)) <= 0)


def test_surface_albedo_textured_two_paths(tmp_path):
    """rt_trace_rays' surface albedo on the camera's rays == rt_render_aov's
    albedo: two kernels instantiations through one shade() and sample_texture"""
    scene, _ = helpers.make_textured_scene(str(tmp_path))
    run = helpers.GpuRun(scene)
    W, H = 48, 32
    rays = rt.camera_rays(run.camera, W, H)
    hits, surf = rt.trace_rays(run.dev, rays, surface=True)
    aov = rt.render_aov(run.dev, run.camera, W, H)
    assert np.array_equal(bits(surf["albedo"]), bits(aov["albedo"].reshape(-1, 3)))
    assert np.array_equal(hits["triangle"], aov["triangle"].reshape(-1))
    # (the loader re-centres the room on its box, which puts this camera in the ceiling's plane: the rays of
    # the upper half of the frame leave the scene, the lower half hits floor, walls and the textured prism)
    assert 0.25 < (hits["triangle"] >= 0).mean() < 0.75
    # textured: the albedo varies inside one triangle
    per_tri = [len(np.unique(bits(surf["albedo"][hits["triangle"] == t]), axis=0)) for t in np.unique(hits["triangle"])]
    assert max(per_tri) > 8, per_tri


# ------------------------------------------------------------------ 5. hazard geometry
@pytest.mark.parametrize("variant", ["degenerate", "duplicate"])
def test_hazard_geometry(tmp_path, variant):
    """zero-area triangles (left out of the BVH, NaN planes in the KD leaves), and
    two identical copies of a quad: two passing tests at exactly the same s —
    the reference keeps the first listed in the leaf, and the bounded
    traversal's unique-minimum shortcut (T*) must step aside"""
    extra = hazards.DEGENERATE_OBJ if variant == "degenerate" else hazards.DUPLICATE_OBJ
    c = _Case(hazards.cornell_variant(str(tmp_path / variant), variant, yaw_room=0.1, extra_obj=extra))
    rays, ref = c.rays("inbox"), c.ref("inbox")
    assert 0.25 <= (ref[:, 0] == 1).mean() <= 0.98
    if variant == "duplicate":  # the duplicated quad (the scene's last 4 triangles) is hit
        ntris = len(c.tris)
        assert ((ref[:, 1] >= ntris - 4) & (ref[:, 0] == 1)).sum() > 50
    for mode in MODES:
        hits, surf = rt.trace_rays(c.run.dev, rays, surface=True, traversal=mode)
        assert_matches_oracle(hits, surf, ref, f"{variant} mode {mode}")


# ------------------------------------------------------------------ 6. camera and AOV
def test_camera_rays_pinhole_model():
    """rt_camera_rays at 40 x 32 on the Cornell camera (yaw 0.1, pitch 0, FOV
    0.8) against a float64 pinhole model of camera_ray's formula with both
    jitter draws 0.5.

    The bound, in units of eps = 2^-24 (one float32 rounding of a value <= 1),
    with the shared sin / cos / tan within 2 ulp = 4 eps (rt_libm.h):
      * px = T * (x + 0.5 - W/2) / (W/2): the parenthesis is exact, T carries
        4 eps, two roundings: 6 eps relative (py alike; the third component is
        exactly 1);
      * normalize: the input error moves the unit vector by at most
        6 eps * |(px, py)| / |v| <= 6 * 0.54 eps (|(px, py)| <= tan(0.4) *
        sqrt(1 + 0.8^2) = 0.54 here); the sum of squares (3 eps), sqrt (1.5 + 1),
        reciprocal (1) and the multiply (1) add 4.5 eps: 7.8 eps;
      * R * dir = (d.x * i + d.y * j) + d.z * k: with pitch 0 an entry of R is
        one trig value (4 eps) or exactly 0 / 1; three products (1 eps each on
        terms whose absolute sum is <= |d| |R_row| = 1) and two additions
        (2 eps): 7.8 + 4 + 1 + 2 = 14.8 eps = 8.8e-7 < 1e-6.
    """
    c = case("cornell")
    cam = c.run.camera
    W, H = 40, 32
    rays = rt.camera_rays(cam, W, H)
    assert rays.shape == (W * H, 6)
    pos = np.array([cam.position.x, cam.position.y, cam.position.z], f32)
    assert np.array_equal(bits(rays[:, :3]), np.broadcast_to(bits(pos), (W * H, 3)))  # the origin, bit for bit
    assert cam.pitch == 0.0
    yaw, pitch, fov = float(cam.yaw), float(cam.pitch), float(cam.FOV)
    Y = np.array([[np.cos(yaw), 0, np.sin(yaw)], [0, 1, 0], [-np.sin(yaw), 0, np.cos(yaw)]])  # columns i, j, k
    X = np.array([[1, 0, 0], [0, np.cos(pitch), -np.sin(pitch)], [0, np.sin(pitch), np.cos(pitch)]])
    R = Y @ X
    T = np.tan(float(f32(fov) / f32(2)))
    ys, xs = np.divmod(np.arange(W * H), W)  # pixel index y*W + x
    v = np.stack([T * (xs + 0.5 - W // 2) / (W // 2), T * (ys + 0.5 - H // 2) / (W // 2), np.ones(W * H)], 1)
    v /= np.linalg.norm(v, axis=1)[:, None]
    want = v @ R.T
    err = np.abs(rays[:, 3:].astype(np.float64) - want).max()
    print(f"camera rays: max |direction - float64 pinhole| = {err:.3e}")
    assert err <= 1e-6, err
    # row 0 is the bottom: the rays of higher rows point further up (world +y; the camera has no roll)
    d = rays[:, 3:].reshape(H, W, 3)
    assert np.all(np.diff(d[:, :, 1], axis=0) > 0)
    # and along a row x grows to the camera's right: R's first column
    assert np.all(np.diff(d @ R[:, 0], axis=1) > 0)


def test_render_aov_equals_camera_rays_plus_trace_rays():
    c = case("room_small")
    W, H = 64, 36
    rays = rt.camera_rays(c.run.camera, W, H)
    ref = c.osc.trace_rays(rays)
    assert 0.5 < (ref[:, 0] == 1).mean()
    for mode in MODES:
        hits, surf = rt.trace_rays(c.run.dev, rays, surface=True, traversal=mode)
        aov = rt.render_aov(c.run.dev, c.run.camera, W, H, traversal=mode)
        assert aov["depth"].shape == (H, W) and aov["normal"].shape == (H, W, 3)
        assert np.array_equal(aov["triangle"].reshape(-1), hits["triangle"])
        assert np.array_equal(bits(aov["depth"].reshape(-1)), bits(surf["t"]))
        assert np.array_equal(bits(aov["normal"].reshape(-1, 3)), bits(surf["normal"]))
        assert np.array_equal(bits(aov["albedo"].reshape(-1, 3)), bits(surf["albedo"]))
        # and the oracle's triangle and normal on those rays
        assert np.array_equal(aov["triangle"].reshape(-1), ref[:, 1].astype(np.int32))
        assert np.array_equal(bits(aov["normal"].reshape(-1, 3)), bits(ref[:, 5:8]))


def test_render_aov_partial_buffers():
    """any AOV buffer may be NULL: the others are written as before"""
    c = case("cornell")
    W, H = 40, 32
    full = rt.render_aov(c.run.dev, c.run.camera, W, H)
    d_depth, d_tri = Dev(np.zeros(W * H, f32)), Dev(np.zeros(W * H, np.int32))
    try:
        b = rt.RtAovBuffers(d_depth.p, None, None, None)
        rt.check(rt.lib().rt_render_aov(c.run.dev.prepared, c.run.camera, W, H, ctypes.byref(b), None))
        b = rt.RtAovBuffers(None, None, None, d_tri.p)
        rt.check(rt.lib().rt_render_aov(c.run.dev.prepared, c.run.camera, W, H, ctypes.byref(b), None))
        assert np.array_equal(bits(d_depth.read()), bits(full["depth"].reshape(-1)))
        assert np.array_equal(d_tri.read(), full["triangle"].reshape(-1))
    finally:
        d_depth.free()
        d_tri.free()


# ------------------------------------------------------------------ 7. coexistence with chained renders
_HIP = None


def _stream():
    global _HIP
    if _HIP is None:
        _HIP = ctypes.CDLL("libamdhip64.so")
    s = ctypes.c_void_p()
    assert _HIP.hipStreamCreate(ctypes.byref(s)) == 0
    return s


def test_query_between_chained_renders():
    """two chained rt_render calls (overlap = 1) with an rt_trace_rays on
    another stream between them: the frame is the one without the query, and
    the query's hits are the oracle's"""
    c = case("room_small")
    W, H, P = 96, 54, 4
    rays, ref = c.rays("inbox"), c.ref("inbox")
    s_render, s_query = _stream(), _stream()

    def frame(with_query):
        g = rt.GBuffer(W, H)
        d_rays, d_hits = Dev(rays), Dev(_guarded(rt.RAY_HIT, N))
        try:
            for k in range(2):
                opt = rt.options(W, H, P, adaptive=False, kernel=rt.KERNEL_WAVEFRONT, overlap=True,
                                 coalesce_passes=-1, stream=s_render.value)
                rt.render(c.run.dev, g, c.run.camera, 0 if k == 0 else 1, opt)
                if with_query and k == 0:
                    rt.trace_rays_device(c.run.dev, d_rays.p, N, d_hits.p, stream=s_query.value)
            rt.join()
            assert _HIP.hipStreamSynchronize(s_query) == 0
            return g.download(), d_hits.read()
        finally:
            d_rays.free()
            d_hits.free()
            g.free()

    plain, _ = frame(False)
    mixed, hits = frame(True)
    helpers.assert_bitwise(mixed, plain, what="chained frame with a query in between")
    assert int(plain[2].sum()) == W * H * P * 2
    assert_matches_oracle(hits[:N], None, ref, "query between chained renders")
    assert (hits[N:].view(np.uint8) == 0xCD).all()
    for s in (s_render, s_query):
        assert _HIP.hipStreamDestroy(s) == 0


def test_two_queries_on_two_streams_equal_serial():
    """rt_trace_rays on one stream and rt_occluded on another, issued back to
    back with nothing between them, share the device's query workspace (ray
    counter, stack spill area): the library orders them on it.  n is twice the
    resident grid's threads (CUs x RQ_WAVES = 4 blocks x 256), so the first
    launch still holds the workspace when the second is enqueued.  Both
    results equal the same calls made one after the other on the null stream."""
    c = case("cornell")
    sa, sb = _stream(), _stream()
    cus = ctypes.c_int(0)
    assert _HIP.hipDeviceGetAttribute(ctypes.byref(cus), 63, 0) == 0  # hipDeviceAttributeMultiprocessorCount
    n = 2 * cus.value * 4 * 256
    assert n > 0
    g = np.random.default_rng(21)
    rays = np.concatenate([_inbox(g, c, n), _unit(g, n)], axis=1).astype(f32)
    d_rays = Dev(rays)
    outs = [Dev(_guarded(rt.RAY_HIT, n)) for _ in range(2)] + [Dev(_guarded(np.dtype(np.uint8), n)) for _ in range(2)]
    (d_hits0, d_hits1, d_occ0, d_occ1) = outs
    try:
        rt.trace_rays_device(c.run.dev, d_rays.p, n, d_hits0.p)
        rt.occluded_device(c.run.dev, d_rays.p, None, n, d_occ0.p)
        rt.trace_rays_device(c.run.dev, d_rays.p, n, d_hits1.p, stream=sa.value)
        rt.occluded_device(c.run.dev, d_rays.p, None, n, d_occ1.p, stream=sb.value)
        assert _HIP.hipStreamSynchronize(sa) == 0 and _HIP.hipStreamSynchronize(sb) == 0
        hits0, hits1, occ0, occ1 = (d.read() for d in outs)
    finally:
        for d in [d_rays] + outs:
            d.free()
        for s in (sa, sb):
            assert _HIP.hipStreamDestroy(s) == 0
    assert np.array_equal(hits1.view(np.uint8), hits0.view(np.uint8)), "rt_trace_rays on a stream vs serial"
    assert np.array_equal(occ1, occ0), "rt_occluded on a stream vs serial"
    assert (hits1[n:].view(np.uint8) == 0xCD).all() and (occ1[n:] == 0xCD).all(), "tail written"
    # the inputs are not trivial, and a ray is occluded (tmax = +inf) exactly where it hits
    hit = hits0["triangle"][:n] >= 0
    assert 0.25 * n < hit.sum() < n
    assert np.array_equal(occ0[:n], hit.astype(np.uint8))


# ------------------------------------------------------------------ 8. torch
def test_torch_tensors_on_the_current_stream():
    """rays in a torch device tensor, the query enqueued on torch's current
    stream (rt.trace_rays_device): the numpy path's hits.  In a child process
    that imports torch first, so torch and the library share one HIP runtime
    (tests/query_torch_child.py)."""
    import sys

    pytest.importorskip("torch")
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "query_torch_child.py")
    r = subprocess.run([sys.executable, child], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout[-2000:] + r.stderr[-4000:]


# ------------------------------------------------------------------ 9. CLI
def _read_pfm(path):
    with open(path, "rb") as f:
        kind = f.readline().strip()
        w, h = (int(v) for v in f.readline().split())
        scale = float(f.readline())
        assert scale < 0  # little-endian
        ch = {b"PF": 3, b"Pf": 1}[kind]
        data = np.frombuffer(f.read(), dtype="<f4")
    assert data.size == w * h * ch
    return data.reshape(h, w, ch) if ch == 3 else data.reshape(h, w)


def test_cli_writes_aov_files(tmp_path):
    """rt_render --aov P: P.albedo.pfm / P.normal.pfm (PF) and P.depth.pfm (Pf),
    rows bottom to top, payloads == rt.render_aov's arrays"""
    exe = os.path.join(os.path.dirname(rt.LIB_PATH), "rt_render")
    W, H = 48, 40
    prefix = str(tmp_path / "aov")
    r = subprocess.run([exe, "--generate", "cornell", str(tmp_path / "scene"), "--width", str(W), "--height", str(H),
                        "--spp", "1", "--passes", "1", "--aov", prefix, "--out", str(tmp_path / "o.png"), "--quiet"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    run = helpers.GpuRun(str(tmp_path / "scene" / "scene.txt"))
    aov = rt.render_aov(run.dev, run.camera, W, H)
    for name in ("albedo", "normal", "depth"):
        got = _read_pfm(prefix + f".{name}.pfm")
        assert got.shape == aov[name].shape
        assert np.array_equal(bits(got), bits(aov[name])), name
    assert np.isinf(aov["depth"]).any() and np.isfinite(aov["depth"]).any()  # the box is open at the front
