"""rt_reproject on the GPU (csrc/reproject.hip): bit-identical to
rt_reproject_host on the synthetic frames of tests/test_reproject_cpu.py and
on real frames of room_small after a small and a large camera move; writes
nothing outside its three output arrays; its result is a G_Buffer the
unchanged renderer continues bit for bit; joins chained renders as rt_tonemap
does; lowers the error of a moving low-spp camera against a 2048-spp
reference; the driver's --reproject-to."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import helpers
import oracle
import reproject_ref as ref
import rt

pytestmark = pytest.mark.gpu
F = np.float32
bits = ref.bits

_HIP = None


def _stream():
    global _HIP
    if _HIP is None:
        _HIP = ctypes.CDLL("libamdhip64.so")
    s = ctypes.c_void_p()
    assert _HIP.hipStreamCreate(ctypes.byref(s)) == 0
    return s


def _assert_same(got, want, what):
    """(fb, sq, count) against (fb, sq, count), any shapes"""
    n = np.asarray(want[2]).size
    cg, cw = np.asarray(got[2]).reshape(n), np.asarray(want[2]).reshape(n)
    assert np.array_equal(cg, cw), f"{what}: {(cg != cw).sum()} counts differ; first {np.nonzero(cg != cw)[0][:4]}"
    for name, a, b, per in (("fb", got[0], want[0], 3), ("sq", got[1], want[1], 1)):
        a, b = bits(a).reshape(n, per), bits(b).reshape(n, per)
        bad = np.nonzero((a != b).any(axis=1))[0]
        assert len(bad) == 0, f"{what}: {len(bad)} {name} pixels differ; first {bad[:4].tolist()}"


def _gpu(src, aov_a, cam_a, aov_b, cam_b, **options):
    """rt.reproject of host arrays -> (fb, sq, count, stats)"""
    H, W = aov_b["depth"].shape
    g = rt.GBuffer(W, H)
    try:
        g.upload(src[0], src[1], src[2], np.zeros(W * H, np.uint32))
        out, stats = rt.reproject(g, aov_a, cam_a, aov_b, cam_b, stats=True, **options)
        try:
            fb, sq, cnt, _ = out.download()
        finally:
            out.free()
    finally:
        g.free()
    return fb, sq, cnt, stats


def _host(src, aov_a, cam_a, aov_b, cam_b, **options):
    return rt.reproject_host(src[0], src[1], src[2], aov_a, cam_a, aov_b, cam_b, stats=True, **options)


# ---------------------------------------------------------------- synthetic frames, bit for bit
@pytest.mark.parametrize("name", ref.CASES)
@pytest.mark.parametrize("shape", ref.SHAPES[:2], ids=lambda s: f"{s[0]}x{s[1]}")
def test_gpu_equals_host(shape, name):
    W, H = shape
    src, aov_a, cam_a, aov_b, cam_b, opts = ref.case(name, W, H)
    got = _gpu(src, aov_a, cam_a, aov_b, cam_b, **opts)
    want = _host(src, aov_a, cam_a, aov_b, cam_b, **opts)
    _assert_same(got, want, f"GPU vs host, {name}")
    assert got[3] == want[3]


@pytest.mark.parametrize("shift", [dict(shift_x=3), dict(shift_y=-3), dict(shift_x=0.5), dict(shift_x=0.37, shift_y=1.6)],
                         ids=["right3", "down3", "half", "oblique"])
def test_gpu_equals_host_on_plane_moves(shift):
    W, H = 67, 45
    src, aov_a, cam_a, aov_b, cam_b = ref.plane_case(W, H, 4.0, **shift)
    got = _gpu(src, aov_a, cam_a, aov_b, cam_b)
    want = _host(src, aov_a, cam_a, aov_b, cam_b)
    _assert_same(got, want, f"GPU vs host, plane {shift}")
    assert got[3] == want[3] and got[3]["kept_pixels"] > W * H // 2


def test_partial_tiles():
    """257 x 3: the ninth 32-pixel tile of a row holds one pixel and five of the tile's eight rows are empty"""
    W, H = 257, 3
    src, aov_a, cam_a, aov_b, cam_b, _ = ref.case("small_move", W, H)
    got = _gpu(src, aov_a, cam_a, aov_b, cam_b)
    want = _host(src, aov_a, cam_a, aov_b, cam_b)
    _assert_same(got, want, "GPU vs host, 257 x 3")
    assert got[3] == want[3] and 0 < got[3]["kept_pixels"] < W * H


# ---------------------------------------------------------------- nothing outside the output
def test_writes_only_its_output():
    W, H = 67, 45
    n = W * H
    pad = 192
    src, aov_a, cam_a, aov_b, cam_b, _ = ref.case("small_move", W, H)
    fill = 0x5A5A5A5A
    d_src = [rt.DeviceArray(a) for a in src]
    d_a = [rt.DeviceArray(aov_a[k]) for k in ("depth", "normal", "triangle")]
    d_b = [rt.DeviceArray(aov_b[k]) for k in ("depth", "normal", "triangle")]
    d_out = [rt.DeviceArray(np.full(pad + n * per + pad, fill, np.uint32)) for per in (3, 1, 1)]
    rng = np.arange(n, dtype=np.uint32) * np.uint32(2654435761)
    d_rng = rt.DeviceArray(rng)
    d_stats = rt.DeviceArray(np.asarray([5, 6, 7, fill], np.uint64))
    everything = d_src + d_a + d_b + d_out + [d_rng, d_stats]
    try:
        gs = rt.G_Buffer(d_src[0].p, d_src[1].p, d_src[2].p, d_rng.p)
        gd = rt.G_Buffer(*[d.p.value + 4 * pad for d in d_out], d_rng.p)
        rt.reproject_device(gs, [d.p for d in d_a], cam_a, [d.p for d in d_b], cam_b, W, H, gd, stats=d_stats.p)
        outs = [d.read() for d in d_out]
        for o in outs:
            assert (o[:pad] == fill).all() and (o[-pad:] == fill).all()
        want = _host(src, aov_a, cam_a, aov_b, cam_b)
        got = (outs[0][pad:-pad].view(F), outs[1][pad:-pad].view(F), outs[2][pad:-pad].view(np.int32))
        _assert_same(got, want, "padded output")
        assert np.array_equal(d_rng.read(), rng)  # random_numbers: neither buffer's is touched
        for d, a in zip(d_src + d_a + d_b, list(src) + [aov_a[k] for k in ("depth", "normal", "triangle")] +
                        [aov_b[k] for k in ("depth", "normal", "triangle")]):
            assert np.array_equal(d.read().view(np.uint32), np.ascontiguousarray(a).view(np.uint32))
        st = d_stats.read()  # the call adds to the three words
        assert [int(v) for v in st] == [5 + n, 6 + want[3]["kept_pixels"], 7 + want[3]["carried_samples"], fill]
    finally:
        for d in everything:
            d.free()


# ---------------------------------------------------------------- real frames
W_REAL, H_REAL, SPP, DEPTH = 96, 64, 4, 8


def _moved(cam, dx=0.0, dy=0.0, dz=0.0, dyaw=0.0, dpitch=0.0):
    return rt.Camera(rt.Vec3D(cam.position.x + dx, cam.position.y + dy, cam.position.z + dz), cam.yaw + dyaw,
                     cam.pitch + dpitch, cam.FOV, cam.aperture_radius)


def _orbit(cam, angle, radius=2.4):
    """the camera turned by `angle` about the vertical axis through the point `radius` in front of it"""
    yaw = cam.yaw + angle
    cx, cz = cam.position.x + radius * np.sin(cam.yaw), cam.position.z + radius * np.cos(cam.yaw)
    return rt.Camera(rt.Vec3D(cx - radius * np.sin(yaw), cam.position.y, cz - radius * np.cos(yaw)), yaw, cam.pitch,
                     cam.FOV, cam.aperture_radius)


@pytest.fixture(scope="module")
def room():
    run = helpers.GpuRun("room_small")
    src, _, g = run.render(W_REAL, H_REAL, SPP, adaptive=False, max_depth=DEPTH)
    cam_a = run.camera
    cam_b = _moved(cam_a, dx=0.08, dz=0.06, dyaw=0.05)  # 0.1 of the 5 x 3 x 4 room, and 0.05 rad
    aov_a = rt.render_aov(run.dev, cam_a, W_REAL, H_REAL)
    aov_b = rt.render_aov(run.dev, cam_b, W_REAL, H_REAL)
    yield run, src, g, cam_a, aov_a, cam_b, aov_b
    g.free()


def _shaped(src):
    fb, sq, cnt = src[:3]
    return fb.reshape(H_REAL, W_REAL, 3), sq.reshape(H_REAL, W_REAL), cnt.reshape(H_REAL, W_REAL)


def test_real_frame_equals_host(room):
    run, src, g, cam_a, aov_a, cam_b, aov_b = room
    n = W_REAL * H_REAL
    out, stats = rt.reproject(g, aov_a, cam_a, aov_b, cam_b, stats=True)
    try:
        got = out.download()
    finally:
        out.free()
    want = _host(_shaped(src), aov_a, cam_a, aov_b, cam_b)
    _assert_same(got, want, "GPU vs host on room_small")
    assert stats == want[3]
    print(f"small move: {stats['kept_pixels'] / n:.3f} of the pixels kept history")
    assert n // 2 < stats["kept_pixels"] < n and stats["carried_samples"] == SPP * stats["kept_pixels"]
    assert np.array_equal(got[3], src[3])  # the new buffer continues the source's RNG streams
    # a half turn: nearly nothing of the old frame is in view
    cam_c = _moved(cam_a, dyaw=np.pi)
    aov_c = rt.render_aov(run.dev, cam_c, W_REAL, H_REAL)
    out, stats = rt.reproject(g, aov_a, cam_a, aov_c, cam_c, stats=True)
    try:
        got = out.download()
    finally:
        out.free()
    want = _host(_shaped(src), aov_a, cam_a, aov_c, cam_c)
    _assert_same(got, want, "GPU vs host after a half turn")
    assert stats == want[3] and stats["kept_pixels"] < n // 10


def test_render_continues_on_the_reprojected_frame(room):
    """rt_render(sample_count = 1, 2 passes) on the reprojected G_Buffer: every count rises by 2 and the sums are
    the oracle's two passes added to the reprojected sums, from the RNG states the first camera's render left"""
    run, src, g, cam_a, aov_a, cam_b, aov_b = room
    n = W_REAL * H_REAL
    out = rt.reproject(g, aov_a, cam_a, aov_b, cam_b)
    try:
        pre = out.download()
        rt.render(run.dev, out, cam_b, 1, rt.options(W_REAL, H_REAL, 2, adaptive=False, max_depth=DEPTH))
        rt.join()
        post = out.download()
    finally:
        out.free()
    assert np.array_equal(post[2], pre[2] + 2)
    assert (pre[2] == 0).any() and (pre[2] == SPP).any()
    fb, sq, cnt, rng = (np.ascontiguousarray(a).copy() for a in pre)
    fb = fb.reshape(n * 3)
    oracle.OracleScene(run.path).render(np.asarray(cam_b.as_list(), F), fb, sq, cnt, rng, W_REAL, H_REAL, 2,
                                        sample_count_arg=1, adaptive=False, max_depth=DEPTH)
    helpers.assert_bitwise(post, (fb.reshape(n, 3), sq, cnt, rng), what="render on the reprojected frame")


def test_reproject_behind_chained_renders(room):
    """rt_reproject behind an open overlap = 1 chain joins it first: the result is that of the same calls
    unchained, and the host twin's"""
    run, _, _, cam_a, aov_a, cam_b, aov_b = room
    W, H, P = W_REAL, H_REAL, 3
    s = _stream()
    d_a = [rt.DeviceArray(aov_a[k]) for k in ("depth", "normal", "triangle")]
    d_b = [rt.DeviceArray(aov_b[k]) for k in ("depth", "normal", "triangle")]

    def frame(chained):
        g, out = rt.GBuffer(W, H), rt.GBuffer(W, H)
        try:
            for k in range(2):
                opt = rt.options(W, H, P, adaptive=False, kernel=rt.KERNEL_WAVEFRONT, overlap=chained,
                                 stream=s.value, max_depth=DEPTH)
                rt.render(run.dev, g, cam_a, 0 if k == 0 else 1, opt)
            if not chained:
                assert _HIP.hipStreamSynchronize(s) == 0
            rt.reproject_device(g.g, [d.p for d in d_a], cam_a, [d.p for d in d_b], cam_b, W, H, out.g,
                                stream=s.value)
            assert _HIP.hipStreamSynchronize(s) == 0
            rt.join()
            return g.download(), out.download()
        finally:
            g.free()
            out.free()

    try:
        src_plain, plain = frame(False)
        src_chained, chained = frame(True)
    finally:
        for d in d_a + d_b:
            d.free()
        assert _HIP.hipStreamDestroy(s) == 0
    helpers.assert_bitwise(src_chained, src_plain, what="chained source frame")
    assert int(src_plain[2].sum()) == W * H * P * 2
    _assert_same(chained, plain, "rt_reproject behind a chain")
    _assert_same(chained, _host(_shaped(src_plain), aov_a, cam_a, aov_b, cam_b), "chained vs host")
    assert (chained[2] == 2 * P).any()


# ---------------------------------------------------------------- quality
def _mse(fb, cnt, ref_mean):
    mean = fb.astype(np.float64) / np.maximum(cnt, 1)[:, None]
    return float(np.mean((mean - ref_mean) ** 2))


def test_moving_camera_error_drops(room):
    """an 8-camera orbit at 4 spp per frame: the last frame's MSE against 2048 spp of the last camera, with the
    history carried from frame to frame and with a reset at every move (the reference's main()).  Measured on
    the MI355X (renders and the reprojection are bit-reproducible, so these are one tree's numbers): reset
    1.91108, reprojected 0.629264, ratio 0.329, 22.0 samples per pixel in the last frame (DESIGN.md "Temporal
    reprojection")."""
    run = room[0]
    W, H, K = W_REAL, H_REAL, 8
    cams = [_orbit(run.camera, -0.02 * k) for k in range(K)]
    opt0 = rt.options(W, H, SPP, adaptive=False, max_depth=DEPTH)
    g = rt.GBuffer(W, H)
    rt.render(run.dev, g, cams[0], 0, opt0)
    aov = rt.render_aov(run.dev, cams[0], W, H)
    kept = []
    for k in range(1, K):
        aov_k = rt.render_aov(run.dev, cams[k], W, H)
        g_k, st = rt.reproject(g, aov, cams[k - 1], aov_k, cams[k], stats=True)
        g.free()
        g, aov = g_k, aov_k
        kept.append(st["kept_pixels"] / (W * H))
        rt.render(run.dev, g, cams[k], 1, opt0)
    rt.join()
    fb, _, cnt, _ = g.download()
    g.free()
    fresh = rt.GBuffer(W, H)
    rt.render(run.dev, fresh, cams[-1], 0, opt0)
    rt.join()
    rfb, _, rcnt, _ = fresh.download()
    for c in range(4):
        rt.render(run.dev, fresh, cams[-1], 0 if c == 0 else 1, rt.options(W, H, 512, adaptive=False, max_depth=DEPTH))
    rt.join()
    tfb, _, tcnt, _ = fresh.download()
    fresh.free()
    assert (tcnt == 2048).all() and (rcnt == SPP).all() and cnt.max() == SPP * K and cnt.min() >= SPP
    truth = tfb.astype(np.float64) / tcnt[:, None]
    e_reset, e_carried = _mse(rfb, rcnt, truth), _mse(fb, cnt, truth)
    print(f"MSE reset {e_reset:.6g} reprojected {e_carried:.6g} ratio {e_carried / e_reset:.6g}; "
          f"kept {min(kept):.3f}..{max(kept):.3f}, mean count {cnt.mean():.2f}")
    assert e_carried < e_reset


# ---------------------------------------------------------------- the driver
def test_cli_reproject(tmp_path):
    exe = os.path.join(os.path.dirname(rt.LIB_PATH), "rt_render")
    W, H = 96, 64
    common = ["--width", str(W), "--height", str(H), "--spp", "4", "--quiet"]
    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir()
    b.mkdir()
    run = helpers.GpuRun("room_small")
    cam_b = _moved(run.camera, dx=0.08, dz=0.06, dyaw=0.05)
    to = " ".join(repr(float(v)) for v in cam_b.as_list()[:5])
    r = subprocess.run([exe, "--generate", "room_small", str(tmp_path / "scene_a")] + common +
                       ["--reproject-to", to, "--spp2", "2", "--denoise", "--out", str(a / "x.png")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe, "--generate", "room_small", str(tmp_path / "scene_b")] + common +
                       ["--out", str(b / "x.png")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe, "--scene", run.path] + common + ["--spp2", "2", "--out", str(b / "y.png")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "usage" in r.stderr  # --spp2 without a camera to move to
    # the same frames through rt.py: the driver's defaults are the wavefront kernel and adaptive sampling
    opt = rt.options(W, H, 4, kernel=rt.KERNEL_WAVEFRONT)
    g = rt.GBuffer(W, H)
    rt.render(run.dev, g, run.camera, 0, opt)
    rt.join()
    rt.save_render(g, str(b / "py.png"))
    assert (b / "x.png").read_bytes() == (b / "py.png").read_bytes()  # without the flag: the frame as it ever was
    out = rt.reproject(g, rt.render_aov(run.dev, run.camera, W, H), run.camera, rt.render_aov(run.dev, cam_b, W, H), cam_b)
    g.free()
    rt.render(run.dev, out, cam_b, 1, rt.options(W, H, 2, kernel=rt.KERNEL_WAVEFRONT))
    rt.join()
    rt.save_render(out, str(a / "py.png"))
    out.free()
    assert (a / "x.png").read_bytes() == (a / "py.png").read_bytes()
    assert (a / "x.png").read_bytes() != (b / "x.png").read_bytes()
    assert (a / "x.denoised.png").exists() and (a / "x.denoised.png").read_bytes() != (a / "x.png").read_bytes()
