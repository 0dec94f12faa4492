"""The path samplers on the GPU (rt_sample_paths, rt_sampler_rays; csrc/query.hip
rt_path_query_kernel<SamplerRays>, rt_sampler_rays_kernel) against their
definition (include/isaklm_rt.h, DESIGN.md §11 "Samplers").

The reference is never the code under test.  The rays are the host twin's
(rt_sampler_rays_host, which tests/test_samplers_cpu.py pins to the numpy
restatement and, for the pinhole, to the oracle's camera sample).  The fused
query is compared with what its contract names: rounds of rt_sampler_rays +
rt_trace_paths (tests/test_gpu_paths.py pins that one to the oracle), and for
the pinhole sampler rt_render and the oracle's or_render themselves.  Every
comparison is bitwise.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import helpers
import independent as ind
import oracle
import path_query_ref as pq
import rt
import test_gpu_paths as tp
import test_gpu_query as tq

pytestmark = pytest.mark.gpu
f32 = np.float32
MODES = tq.MODES
W, H = 96, 54
APP = os.path.join(helpers.ROOT, "isaklm-raytracer_amd", "rt_render")
IMAGE = ["pinhole", "equirect", "fisheye", "ortho"]
ORTHO_HALF = 1.5


def image_sampler(c, kind, pixels=None, width=W, height=H):
    """the scene's own camera under each model (fisheye: its FOV across the image circle); the panorama of the
    Cornell box, whose camera looks in from outside, is taken from a point inside the box"""
    cam = c.run.camera
    if kind == "equirect" and "cornell" in c.run.path:
        cam = rt.Camera()
        cam.position.x, cam.position.y, cam.position.z = -0.21, 0.9, 0.13
        cam.yaw, cam.pitch, cam.FOV, cam.aperture_radius = 0.4, -0.1, 1.0, 0.0
    return rt.Sampler(kind, width, height, cam, ortho_half_width=ORTHO_HALF, pixels=pixels)


_points = {}


def surface_points(c):
    """(m, 6) positions and normals: the rt_trace_rays surface hits of the frame's pixel-centre rays"""
    if c.run.path not in _points:
        rays = rt.sampler_rays_host(image_sampler(c, "pinhole"))
        hits, surf = rt.trace_rays(c.run.dev, rays, surface=True)
        ok = hits["triangle"] >= 0
        assert ok.mean() > 0.5
        pts = np.concatenate([surf["position"][ok], surf["normal"][ok]], axis=1).astype(f32)
        pts.setflags(write=False)
        _points[c.run.path] = pts
    return _points[c.run.path]


def make_sampler(c, kind, n=None):
    """a sampler of `kind` with n elements (None: the whole frame / every surface point); image kinds get a
    pixel list spread over the frame"""
    if kind == "hemisphere":
        pts = surface_points(c)
        return rt.Sampler("hemisphere", points=pts if n is None else pts[(np.arange(n) * 19 + 7) % len(pts)])
    if n is None:
        return image_sampler(c, kind)
    return image_sampler(c, kind, pixels=((np.arange(n) * 19 + 7) % (W * H)).astype(np.int32))


# ------------------------------------------------------------------ 1. rays
OFF, PAD = 5, 131


def guarded(values, n, width, dtype):
    a = np.frombuffer(bytes([0xA5]) * ((OFF + n + PAD) * width * 4), dtype=dtype).copy()
    if values is not None:
        a[OFF * width:(OFF + n) * width] = np.asarray(values, dtype).reshape(-1)
    return a


def assert_guards(after, before, n, width, what):
    lo, hi = OFF * width, (OFF + n) * width
    assert np.array_equal(after[:lo].view(np.uint32), before[:lo].view(np.uint32)), what + ": before the first record"
    assert np.array_equal(after[hi:].view(np.uint32), before[hi:].view(np.uint32)), what + ": past the n-th record"
    return after[lo:hi]


def device_rays(smp, rng):
    """rt_sampler_rays on buffers inside guard words; the pixel list / points sit in exact-size buffers"""
    n = smp.n
    h_rays, h_rng = guarded(None, n, 6, f32), guarded(rng, n, 1, np.uint32)
    d_rays, d_rng = tq.Dev(h_rays), tq.Dev(h_rng)
    d_pix = tq.Dev(smp.pixels) if smp.pixels is not None else None
    d_pts = tq.Dev(smp.points) if smp.points is not None else None
    try:
        s = smp.struct(d_pix.p if d_pix else None, d_pts.p if d_pts else None)
        rt.check(rt.lib().rt_sampler_rays(ctypes.byref(s), d_rng.p.value + 4 * OFF if rng is not None else None, n,
                                          d_rays.p.value + 24 * OFF, None))
        rays = assert_guards(d_rays.read(), h_rays, n, 6, "rays").reshape(n, 6)
        out = assert_guards(d_rng.read(), h_rng, n, 1, "rng")
        for d, a in ((d_pix, smp.pixels), (d_pts, smp.points)):
            if d:
                assert np.array_equal(d.read().view(np.uint32), np.ascontiguousarray(a).view(np.uint32)), "input written"
    finally:
        for d in (d_rays, d_rng, d_pix, d_pts):
            if d:
                d.free()
    return rays, out


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
@pytest.mark.parametrize("kind", IMAGE + ["hemisphere"])
def test_rays_equal_the_host_twin(kind, n):
    c = tq.case("cornell")
    smp = make_sampler(c, kind, n)
    if kind != "hemisphere" and n >= 63:  # entries outside the frame among them
        smp.pixels[[3, 10, 40, 62]] = [-1, W * H, np.iinfo(np.int32).min, np.iinfo(np.int32).max]
    st = oracle.mt19937(n, skip=11)
    rays, out = device_rays(smp, st)
    want_rays, want_out = rt.sampler_rays_host(smp, st)
    assert np.array_equal(rays.view(np.uint32), want_rays.view(np.uint32)), np.nonzero(rays != want_rays)
    assert np.array_equal(out, want_out)
    if n:
        assert (out != st).any()
    if kind != "hemisphere":  # the centre rays: no RNG
        rays, out = device_rays(smp, None)
        assert np.array_equal(rays.view(np.uint32), rt.sampler_rays_host(smp).view(np.uint32))
        assert (out.view(np.uint8) == 0xA5).all()


def test_whole_frames_and_the_pinhole_centre_rays():
    c = tq.case("cornell")
    st = oracle.mt19937(W * H)
    for kind in IMAGE:
        smp = image_sampler(c, kind)
        rays, out = rt.sampler_rays(smp, st)
        want = rt.sampler_rays_host(smp, st)
        assert np.array_equal(rays.view(np.uint32), want[0].view(np.uint32)) and np.array_equal(out, want[1]), kind
    centre = rt.sampler_rays(image_sampler(c, "pinhole"))
    assert np.array_equal(centre.view(np.uint32), rt.camera_rays(c.run.camera, W, H).view(np.uint32))
    # the pinhole's samples are the renderer's camera samples (the restatement pinned to the oracle)
    rays, out = rt.sampler_rays(image_sampler(c, "pinhole"), st)
    want = pq.camera_samples(c.osc.camera, W, H, st)
    assert np.array_equal(rays.view(np.uint32), want[0].view(np.uint32)) and np.array_equal(out, want[1])


# ------------------------------------------------------------------ 2. frames: the pinhole sampler is rt_render
def sampled_frame(c, smp, samples, mode, gb=None, accumulate=False):
    """rt_sample_paths on a G_Buffer's four arrays -> (fb, sq, count, rng), and the call's stats"""
    own = gb is None
    gb = gb or rt.GBuffer(smp.width, smp.height)
    d_stats = tq.Dev(np.zeros(5, np.uint64))
    try:
        rt.sample_paths_device(c.run.dev, smp, gb.g.random_numbers, gb.n, gb.g.frame_buffer, gb.g.squared_luminance,
                               gb.g.sample_count, samples=samples, accumulate=accumulate, traversal=mode,
                               stats_ptr=d_stats.p)
        return gb.download(), dict(zip(rt.PATH_STATS, (int(v) for v in d_stats.read())))
    finally:
        d_stats.free()
        if own:
            gb.free()


@pytest.mark.parametrize("name", ["cornell", "room_small"])
def test_pinhole_frames_equal_rt_render(name):
    c = tq.case(name)
    smp = image_sampler(c, "pinhole")
    ref1, k = tp.oracle_frame(c.run.path, W, H)
    tp.check_reference_is_not_trivial(ref1, k, W, H, name)
    renders = {kernel: c.run.render(W, H, 3, kernel=kernel)[0] for kernel in (rt.KERNEL_MEGA, rt.KERNEL_WAVEFRONT)}
    for mode in MODES:
        got, stats = sampled_frame(c, smp, 3, mode)
        for kernel, frame in renders.items():
            helpers.assert_bitwise(got, frame, what=f"{name} mode {mode}: 3 samples vs rt_render kernel {kernel}")
        assert (got[2] == 3).all() and stats["rays"] == W * H and stats["paths"] == 3 * W * H
        one, stats = sampled_frame(c, smp, 1, mode)
        pq.assert_same((one[0], one[1], one[3]), ref1, f"{name} mode {mode}: 1 sample vs the oracle's frame")
        assert (one[2] == 1).all()
        tp.assert_stats(stats, k, W * H)
    # and continued: 2 more samples on the 1-sample frame = rt_render's 3 passes
    gb = rt.GBuffer(W, H)
    try:
        sampled_frame(c, smp, 1, MODES[0], gb)
        got, _ = sampled_frame(c, smp, 2, MODES[0], gb, accumulate=True)
    finally:
        gb.free()
    helpers.assert_bitwise(got, renders[rt.KERNEL_WAVEFRONT], what=f"{name}: 1 + 2 accumulated samples vs rt_render")


# ------------------------------------------------------------------ 3. the contract: fused == unfused rounds
def unfused(c, smp, rng, rounds, mode, start=None):
    rad, sq = (None, None) if start is None else start
    for _ in range(rounds):
        rays, rng = rt.sampler_rays(smp, rng)
        rad, sq, rng = rt.trace_paths(c.run.dev, rays, rng, samples=1, traversal=mode, radiance=rad, sq=sq)
    return rad, sq, rng


@pytest.mark.parametrize("kind", ["equirect", "fisheye", "ortho", "hemisphere"])
def test_fused_equals_unfused_rounds(kind):
    c = tq.case("cornell")
    smp = make_sampler(c, kind)
    n = smp.n
    assert n > 2000
    st = oracle.mt19937(n, skip=5)
    for mode in MODES:
        rad, sq, rng, cnt = rt.sample_paths(c.run.dev, smp, st, samples=4, traversal=mode, count=True)
        want = unfused(c, smp, st, 4, mode)
        pq.assert_same((rad, sq, rng), want, f"{kind} mode {mode}: 4 fused samples vs 4 rounds")
        assert (cnt == 4).all()
        lit = (rad != 0).any(axis=1)
        assert lit.mean() > 0.10, (kind, lit.mean())
        # the samples really differ: the sum is not 4 times the first sample
        first = rt.sample_paths(c.run.dev, smp, st, samples=1, traversal=mode)
        pq.assert_same(first, unfused(c, smp, st, 1, mode), f"{kind} mode {mode}: 1 sample")
        assert (rad[lit] != first[0][lit] * f32(4)).any(axis=1).mean() > 0.5
        # accumulate = 1: onto an earlier call's sums and counts
        old_cnt = (np.arange(n) % 7).astype(np.int32)
        rad2, sq2, rng2, cnt2 = rt.sample_paths(c.run.dev, smp, first[2], samples=4, traversal=mode, radiance=first[0],
                                                sq=first[1], count=old_cnt)
        want = unfused(c, smp, first[2], 4, mode, start=(first[0], first[1]))
        pq.assert_same((rad2, sq2, rng2), want, f"{kind} mode {mode}: 4 accumulated samples vs 4 rounds")
        assert np.array_equal(cnt2, old_cnt + 4)


def test_hemisphere_probe_gathers_light():
    """cosine-weighted probes on the Cornell box's surfaces: light arrives at most of them, from their own side"""
    c = tq.case("cornell")
    pts = surface_points(c)
    smp = rt.Sampler("hemisphere", points=pts)
    rays, _ = rt.sampler_rays(smp, oracle.mt19937(len(pts)))
    cos = np.einsum("ij,ij->i", rays[:, 3:].astype(np.float64), pts[:, 3:].astype(np.float64))
    assert cos.min() >= -1e-6 and np.array_equal(rays[:, :3], pts[:, :3])
    rad, _, _ = rt.sample_paths(c.run.dev, smp, oracle.mt19937(len(pts)), samples=8)
    assert (rad != 0).any(axis=1).mean() > 0.5 and np.isfinite(rad).all()


# ------------------------------------------------------------------ 4. pixel lists and edge cases
@pytest.mark.parametrize("kind", IMAGE)
def test_pixel_list_entries_outside_the_frame(kind):
    c = tq.case("cornell")
    i32 = np.iinfo(np.int32)
    n = 200
    pix = ((np.arange(n) * 19 + 7) % (W * H)).astype(np.int32)
    bad = np.array([0, 3, 64, 65, 130, 199])
    pix[bad] = [-1, W * H, i32.min, i32.max, W * H + 5, -W * H]
    pix[7] = pix[8]  # a repeated pixel: two elements, each with its own state
    smp = image_sampler(c, kind, pixels=pix)
    st = oracle.mt19937(n, skip=3)
    inside = np.ones(n, bool)
    inside[bad] = False
    whole = rt.sample_paths(c.run.dev, image_sampler(c, kind), oracle.mt19937(W * H), samples=1)
    for mode in MODES:
        rad, sq, rng, cnt = rt.sample_paths(c.run.dev, smp, st, samples=2, traversal=mode, count=True)
        assert (rad[bad].view(np.uint32) == 0).all() and (sq[bad].view(np.uint32) == 0).all()  # +0
        assert np.array_equal(rng[bad], st[bad]) and (cnt == 2).all()
        pq.assert_same((rad, sq, rng), unfused(c, smp, st, 2, mode), f"{kind} mode {mode}: list vs rounds")
        assert (rng[inside] != st[inside]).all()
        # accumulate = 1: the old sums stay where the element lies outside the frame
        old = (np.full((n, 3), 0.25, f32), np.full(n, 0.5, f32))
        rad2, sq2, rng2, cnt2 = rt.sample_paths(c.run.dev, smp, st, samples=2, traversal=mode, radiance=old[0], sq=old[1],
                                                count=np.full(n, 9, np.int32))
        assert (rad2[bad] == f32(0.25)).all() and (sq2[bad] == f32(0.5)).all() and np.array_equal(rng2[bad], st[bad])
        assert (cnt2 == 11).all() and np.array_equal(rng2, rng)
    # a listed pixel is the frame's pixel: the whole frame's first sample from the same states
    sub = np.array([5, 17, 17, W * H - 1], np.int32)
    got = rt.sample_paths(c.run.dev, image_sampler(c, kind, pixels=sub), oracle.mt19937(W * H)[sub], samples=1)
    pq.assert_same(got, tuple(a[sub] for a in whole), f"{kind}: listed pixels vs the frame")


def test_fisheye_corner_pixels():
    """outside the image circle: L = 0, and the RNG is advanced by exactly the sampler's 2 draws per sample"""
    c = tq.case("cornell")
    corners = np.array([0, W - 1, (H - 1) * W, W * H - 1, 1, W], np.int32)
    centre = np.array([(H // 2) * W + W // 2], np.int32)
    pix = np.concatenate([corners, centre])
    st = oracle.mt19937(len(pix), skip=21)
    for mode in MODES:
        rad, sq, rng, cnt = rt.sample_paths(c.run.dev, image_sampler(c, "fisheye", pixels=pix), st, samples=3,
                                            traversal=mode, count=True)
        want = st[:len(corners)].copy()
        for _ in range(3 * 2):
            _, want = ind.rng_next(want)
        assert np.array_equal(rng[:len(corners)], want)
        assert (rad[:len(corners)].view(np.uint32) == 0).all() and (sq[:len(corners)].view(np.uint32) == 0).all()
        assert (cnt == 3).all()
        assert rng[-1] != st[-1]


def test_nan_camera_misses():
    """a camera of NaN and infinite fields: every ray misses, L = 0, only the sampler's draws move the RNG"""
    c = tq.case("cornell")
    cam = rt.Camera()
    cam.position.x, cam.position.y, cam.position.z = float("nan"), 0.0, float("inf")
    cam.yaw, cam.pitch, cam.FOV, cam.aperture_radius = float("nan"), float("inf"), 1.0, float("nan")
    st = oracle.mt19937(W * H)
    for kind, draws in (("pinhole", 4), ("equirect", 2), ("fisheye", 2), ("ortho", 2)):
        smp = rt.Sampler(kind, W, H, cam, ortho_half_width=1.0)
        rad, sq, rng = rt.sample_paths(c.run.dev, smp, st, samples=2)
        want = st.copy()
        for _ in range(2 * draws):
            _, want = ind.rng_next(want)
        assert (rad.view(np.uint32) == 0).all() and (sq.view(np.uint32) == 0).all() and np.array_equal(rng, want), kind


# ------------------------------------------------------------------ 5. more elements than resident lanes
def test_more_elements_than_resident_lanes():
    """a 600 x 500 frame, 2 samples: every lane takes new elements many times and draws each one's second ray
    where its first path ended"""
    c = tq.case("cornell")
    w, h = 600, 500
    got, stats = sampled_frame(c, image_sampler(c, "pinhole", width=w, height=h), 2, rt.TRAVERSAL_BOUNDED)
    want = c.run.render(w, h, 2, kernel=rt.KERNEL_WAVEFRONT)[0]
    helpers.assert_bitwise(got, want, what="600 x 500 x 2 samples vs rt_render")
    assert stats["rays"] == w * h and stats["paths"] == 2 * w * h
    assert (got[0] != 0).any(axis=1).mean() > 0.10


# ------------------------------------------------------------------ 6. between chained renders
def test_sample_paths_between_chained_renders():
    """two chained rt_render calls (overlap = 1) with an rt_sample_paths on another stream between them: the
    frame is the one without the query, and the query's outputs are the standalone ones"""
    c = tq.case("room_small")
    P = 4
    n = W * H
    smp = image_sampler(c, "equirect")
    st = oracle.mt19937(n, skip=2)
    alone = rt.sample_paths(c.run.dev, smp, st, samples=2, count=True)
    assert (alone[0] != 0).any(axis=1).mean() > 0.10
    s_render, s_query = tq._stream(), tq._stream()

    def frame(with_query):
        gb = rt.GBuffer(W, H)
        d_rng = tq.Dev(np.concatenate([st, np.full(64, 0xA5A5A5A5, np.uint32)]))
        d_rad, d_sq = tq.Dev(np.full(3 * n + 64, -7.0, f32)), tq.Dev(np.full(n + 64, -7.0, f32))
        d_cnt = tq.Dev(np.full(n + 64, -7, np.int32))
        try:
            for k in range(2):
                opt = rt.options(W, H, P, adaptive=False, kernel=rt.KERNEL_WAVEFRONT, overlap=True,
                                 coalesce_passes=-1, stream=s_render.value)
                rt.render(c.run.dev, gb, c.run.camera, 0 if k == 0 else 1, opt)
                if with_query and k == 0:
                    rt.sample_paths_device(c.run.dev, smp, d_rng.p, n, d_rad.p, d_sq.p, d_cnt.p, samples=2,
                                           stream=s_query.value)
            rt.join()
            assert tq._HIP.hipStreamSynchronize(s_query) == 0
            return gb.download(), d_rad.read(), d_sq.read(), d_rng.read(), d_cnt.read()
        finally:
            for d in (d_rng, d_rad, d_sq, d_cnt):
                d.free()
            gb.free()

    plain = frame(False)[0]
    mixed, rad, sq, rng, cnt = frame(True)
    helpers.assert_bitwise(mixed, plain, what="chained frame with a sampled query in between")
    assert int(plain[2].sum()) == n * P * 2
    pq.assert_same((rad[:3 * n].reshape(n, 3), sq[:n], rng[:n]), alone[:3], "the sampled query between chained renders")
    assert np.array_equal(cnt[:n], alone[3]) and (cnt[:n] == 2).all()
    assert (rad[3 * n:] == f32(-7.0)).all() and (sq[n:] == f32(-7.0)).all() and (rng[n:] == 0xA5A5A5A5).all()
    assert (cnt[n:] == -7).all()
    for s in (s_render, s_query):
        assert tq._HIP.hipStreamDestroy(s) == 0


# ------------------------------------------------------------------ 7. the driver
def drive(args, tmp_path, name, scene="cornell"):
    out = tmp_path / name
    scene = helpers.scene_path(scene)
    r = subprocess.run([APP, "--scene", scene, "--width", str(W), "--height", str(H), "--spp", "4", "--quiet", "--out",
                        str(out)] + args, capture_output=True, text=True, timeout=150)
    return r, out


def test_driver_camera_models(tmp_path):
    plain, p_out = drive(["--adaptive", "0"], tmp_path, "plain.png")
    pin, s_out = drive(["--adaptive", "0", "--camera-model", "pinhole"], tmp_path, "pinhole.png")
    assert plain.returncode == 0 and pin.returncode == 0, plain.stderr + pin.stderr
    assert p_out.read_bytes() == s_out.read_bytes()
    # in calls of 3 + 1 samples, through a checkpoint: the same frame
    a, _ = drive(["--camera-model", "pinhole", "--passes", "3", "--spp", "3", "--checkpoint", str(tmp_path / "g.ckpt")],
                 tmp_path, "three.png")
    b, r_out = drive(["--camera-model", "pinhole", "--passes", "3", "--resume", str(tmp_path / "g.ckpt")], tmp_path,
                     "resumed.png")
    assert a.returncode == 0 and b.returncode == 0, a.stderr + b.stderr
    assert r_out.read_bytes() == p_out.read_bytes()
    # the panorama wraps: the left and right edge columns are neighbours, the left and middle ones are not
    eq, e_out = drive(["--camera-model", "equirect", "--spp", "32"], tmp_path, "equirect.png", scene="room_small")
    assert eq.returncode == 0, eq.stderr
    img = rt.decode_image(str(e_out)).astype(np.float64)[:, :, :3]
    assert img.shape == (H, W, 3) and img.std() > 5
    seam = np.abs(img[:, 0] - img[:, -1]).mean()
    across = np.abs(img[:, 0] - img[:, W // 2]).mean()
    print(f"equirect seam {seam:.2f} vs left-middle {across:.2f}")
    assert seam < across
    for model in ("fisheye", "ortho"):
        r, out = drive(["--camera-model", model, "--ortho-half-width", "1.5"], tmp_path, model + ".png")
        assert r.returncode == 0, r.stderr
        assert rt.decode_image(str(out)).shape == (H, W, 4) and out.read_bytes() != p_out.read_bytes()


@pytest.mark.parametrize("args", [
    ["--camera-model", "pinhole", "--adaptive", "1"],
    ["--camera-model", "equirect", "--shard", "0", "2"],
    ["--camera-model", "pinhole", "--reproject-to", "0 1 0 0 0"],
    ["--camera-model", "fisheye", "--aov", "x"],
    ["--camera-model", "ortho", "--denoise"],
    ["--camera-model", "cylindrical"],
])
def test_driver_usage_errors(tmp_path, args):
    r, out = drive(args, tmp_path, "never.png")
    assert r.returncode == 2 and "usage: rt_render" in r.stderr and not out.exists()
