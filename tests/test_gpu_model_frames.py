"""AOVs, denoising and reprojection for every camera model on the GPU (rt_sample_aov, rt_denoise_sampler,
rt_reproject_sampler; include/isaklm_rt.h "frames of every camera model").

The reference is never the code under test: rt_sample_aov is compared with what its contract names
(rt_sampler_rays + rt_trace_rays, which tests/test_gpu_query.py pins to the oracle, and rt_render_aov), the
denoiser and the reprojection with their host twins (which tests/test_model_frames_cpu.py pins to their
properties and to the existing calls).  Every comparison is bitwise; the one quality test compares two measured
errors."""
import ctypes

import numpy as np
import pytest

import denoise_ref as dref
import helpers
import model_frames_ref as mf
import rt
import test_gpu_query as tq

pytestmark = pytest.mark.gpu
F = np.float32
bits = mf.bits
W, H = 67, 45
DEPTH = 8
FILL = 0x5A5A5A5A


def scene_sampler(c, kind, width=W, height=H, pixels=None, move=None):
    """the scene's own camera under each model (fisheye: 3 rad across the image circle); move: (dx, dz, dyaw)"""
    cam = c.run.camera
    dx, dz, dyaw = move or (0.0, 0.0, 0.0)
    cam = rt.Camera(rt.Vec3D(cam.position.x + dx, cam.position.y, cam.position.z + dz), cam.yaw + dyaw, cam.pitch,
                    3.0 if kind == "fisheye" else cam.FOV, 0.0)
    return rt.Sampler(kind, width, height, cam, ortho_half_width=1.5, pixels=pixels)


def aov_of_rays(c, smp, mode):
    """the contract's other side: rt_sampler_rays(rng = NULL) + rt_trace_rays with a surface output"""
    hits, surf = rt.trace_rays(c.run.dev, rt.sampler_rays(smp), surface=True, traversal=mode)
    return dict(depth=surf["t"], normal=surf["normal"], albedo=surf["albedo"], triangle=hits["triangle"])


def assert_aov_equal(got, want, what):
    for name in ("depth", "normal", "albedo", "triangle"):
        a = np.ascontiguousarray(got[name]).reshape(-1).view(np.uint32)
        b = np.ascontiguousarray(want[name]).reshape(-1).view(np.uint32)
        assert a.shape == b.shape and np.array_equal(a, b), f"{what}: {name}: {(a != b).sum()} words differ"


# ---------------------------------------------------------------- rt_sample_aov
@pytest.mark.parametrize("mode", tq.MODES, ids=["bounded", "kd"])
@pytest.mark.parametrize("kind", mf.KINDS)
def test_sample_aov_equals_rays_plus_trace(kind, mode):
    c = tq.case("room_small")
    smp = scene_sampler(c, kind)
    got = rt.sample_aov(c.run.dev, smp, traversal=mode)
    assert got["depth"].shape == (H, W) and got["normal"].shape == (H, W, 3) and got["triangle"].dtype == np.int32
    assert_aov_equal(got, aov_of_rays(c, smp, mode), kind)
    hit = got["triangle"] >= 0
    assert hit.mean() > 0.3 and np.isfinite(got["depth"][hit]).all()
    assert np.isinf(got["depth"][~hit]).all() and not got["normal"][~hit].any() and not got["albedo"][~hit].any()
    if kind == "fisheye":  # the pixels outside the image circle miss
        assert (~hit[~mf.in_frame(smp)]).all() and (~mf.in_frame(smp)).sum() > 0
    if kind == "pinhole":
        assert_aov_equal(got, rt.render_aov(c.run.dev, smp.camera, W, H, traversal=mode), "pinhole vs rt_render_aov")


@pytest.mark.parametrize("kind", mf.KINDS)
def test_sample_aov_pixel_list(kind):
    c = tq.case("room_small")
    pixels = ((np.arange(200) * 19 + 7) % (W * H)).astype(np.int32)
    pixels[[3, 77]] = -1
    pixels[[0, 150]] = W * H
    pixels[[10, 11, 199]] = pixels[9]
    smp = scene_sampler(c, kind, pixels=pixels)
    got = rt.sample_aov(c.run.dev, smp)
    assert got["depth"].shape == (200,) and got["albedo"].shape == (200, 3)
    assert_aov_equal(got, aov_of_rays(c, smp, None), kind)
    frame = rt.sample_aov(c.run.dev, scene_sampler(c, kind))
    inside = (pixels >= 0) & (pixels < W * H)
    assert (got["triangle"][~inside] == -1).all() and np.isinf(got["depth"][~inside]).all()
    assert np.array_equal(got["triangle"][inside], frame["triangle"].reshape(-1)[pixels[inside]])
    assert np.array_equal(bits(got["depth"])[inside], bits(frame["depth"]).reshape(-1)[pixels[inside]])


@pytest.mark.parametrize("n", [1, 65])
def test_sample_aov_writes_only_n_records_and_adds_stats(n):
    c = tq.case("room_small")
    pad = 96
    pixels = ((np.arange(n) * 31 + W * (H // 2)) % (W * H)).astype(np.int32)
    smp = scene_sampler(c, "equirect", pixels=pixels)
    want = aov_of_rays(c, smp, None)
    outs = [tq.Dev(np.full(pad + n * per + pad, FILL, np.uint32)) for per in (1, 3, 3, 1)]
    d_pix, d_st = tq.Dev(pixels), tq.Dev(np.asarray([5, 6, 7, FILL], np.uint64))
    try:
        ptrs = [d.p.value + 4 * pad for d in outs]
        rt.sample_aov_device(c.run.dev, smp, n, ptrs, stats_ptr=d_st.p, pixels_ptr=d_pix.p)
        got = [d.read() for d in outs]
        for o in got:
            assert (o[:pad] == FILL).all() and (o[-pad:] == FILL).all()
        got = dict(zip(("depth", "normal", "albedo", "triangle"), (o[pad:-pad] for o in got)))
        assert_aov_equal(got, want, f"n = {n}")
        hits = int((want["triangle"] >= 0).sum())
        st = [int(v) for v in d_st.read()]
        assert st[:2] == [5 + n, 6 + hits] and 7 <= st[2] <= 7 + n and st[3] == FILL
        # only what is asked for is written: the triangle ids alone, then nothing at all
        only = tq.Dev(np.full(n + 2 * pad, FILL, np.uint32))
        try:
            rt.sample_aov_device(c.run.dev, smp, n, [None, None, None, only.p.value + 4 * pad], pixels_ptr=d_pix.p)
            o = only.read()
            assert (o[:pad] == FILL).all() and (o[-pad:] == FILL).all()
            assert np.array_equal(o[pad:-pad].view(np.int32), want["triangle"])
            rt.sample_aov_device(c.run.dev, smp, n, [None, None, None, None], pixels_ptr=d_pix.p)
            rt.sample_aov_device(c.run.dev, smp, 0, ptrs, pixels_ptr=d_pix.p)
        finally:
            only.free()
    finally:
        for d in outs + [d_pix, d_st]:
            d.free()


def test_sample_aov_between_chained_renders():
    """two chained rt_render calls (overlap = 1) with an rt_sample_aov on another stream between them: the frame
    is the one without the query, and the query's buffers are the standalone ones"""
    c = tq.case("room_small")
    w, h, P = 96, 54, 4
    n = w * h
    smp = scene_sampler(c, "equirect", w, h)
    alone = rt.sample_aov(c.run.dev, smp)
    s_render, s_query = tq._stream(), tq._stream()

    def frame(with_query):
        g = rt.GBuffer(w, h)
        outs = [tq.Dev(np.full(n * per + 64, FILL, np.uint32)) for per in (1, 3, 3, 1)]
        try:
            for k in range(2):
                opt = rt.options(w, h, P, adaptive=False, kernel=rt.KERNEL_WAVEFRONT, overlap=True,
                                 coalesce_passes=-1, stream=s_render.value)
                rt.render(c.run.dev, g, c.run.camera, 0 if k == 0 else 1, opt)
                if with_query and k == 0:
                    rt.sample_aov_device(c.run.dev, smp, n, [d.p for d in outs], stream=s_query.value)
            rt.join()
            assert tq._HIP.hipStreamSynchronize(s_query) == 0
            return g.download(), [d.read() for d in outs]
        finally:
            for d in outs:
                d.free()
            g.free()

    plain, _ = frame(False)
    mixed, outs = frame(True)
    helpers.assert_bitwise(mixed, plain, what="chained frame with rt_sample_aov in between")
    assert int(plain[2].sum()) == n * P * 2
    for o, per in zip(outs, (1, 3, 3, 1)):
        assert (o[n * per:] == FILL).all()
    got = dict(zip(("depth", "normal", "albedo", "triangle"), (o[:n * per] for o, per in zip(outs, (1, 3, 3, 1)))))
    assert_aov_equal(got, alone, "rt_sample_aov between chained renders")
    for s in (s_render, s_query):
        assert tq._HIP.hipStreamDestroy(s) == 0


# ---------------------------------------------------------------- rt_denoise_sampler
def _gpu_denoise(f, smp, **options):
    Hf, Wf = f["count"].shape
    g = rt.GBuffer(Wf, Hf)
    try:
        g.upload(f["fb"], f["sq"], f["count"], np.zeros(Wf * Hf, np.uint32))
        return rt.denoise_sampler(g, f, smp, **options)
    finally:
        g.free()


def _host_denoise(f, smp, **options):
    return rt.denoise_sampler_host(f["fb"], f["sq"], f["count"], f["depth"], f["normal"], f["albedo"], smp, **options)


@pytest.mark.parametrize("demodulate", [True, False], ids=["demodulated", "plain"])
@pytest.mark.parametrize("kind", ["equirect", "fisheye"])
@pytest.mark.parametrize("shape", [(67, 45), (257, 3), (5, 4)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_denoise_sampler_equals_host(shape, kind, demodulate):
    """257 x 3: partial tiles; 5 x 4 at 5 levels: 2 * step >= width, the wrapped taps alias pixels"""
    w, h = shape
    f = dref.synthetic_frame(w, h)
    smp = mf.sampler(kind, w, h)
    got = _gpu_denoise(f, smp, iterations=5, demodulate=demodulate)
    want = _host_denoise(f, smp, iterations=5, demodulate=demodulate)
    assert got.shape == (h, w, 3) and np.array_equal(bits(got), bits(want))
    clamped = rt.denoise_host(f["fb"], f["sq"], f["count"], f["depth"], f["normal"], f["albedo"], iterations=5,
                              demodulate=demodulate)
    assert np.array_equal(bits(got), bits(clamped)) == (kind != "equirect")


def _sampled_gbuffer(c, smp, spp, g=None, accumulate=False):
    g = g or rt.GBuffer(smp.width, smp.height)
    rt.sample_paths_device(c.run.dev, smp, g.g.random_numbers, smp.n, g.g.frame_buffer, g.g.squared_luminance,
                           g.g.sample_count, samples=spp, max_depth=DEPTH, accumulate=accumulate)
    return g


def test_denoise_sampler_real_panorama():
    """a 96 x 48 panorama of room_small at 4 spp, guides from rt_sample_aov: GPU == host, and the GPU's filter
    commutes with a roll of the frame's columns"""
    c = tq.case("room_small")
    w, h = 96, 48
    smp = scene_sampler(c, "equirect", w, h)
    aov = rt.sample_aov(c.run.dev, smp)
    g = _sampled_gbuffer(c, smp, 4)
    try:
        fb, sq, cnt, _ = g.download()
        base = rt.denoise_sampler(g, aov, smp)
    finally:
        g.free()
    f = dict(fb=fb.reshape(h, w, 3), sq=sq.reshape(h, w), count=cnt.reshape(h, w), depth=aov["depth"],
             normal=aov["normal"], albedo=aov["albedo"])
    assert (cnt == 4).all() and np.isfinite(base).all() and (base != 0).any(axis=2).mean() > 0.5
    assert np.array_equal(bits(base), bits(_host_denoise(f, smp)))
    noisy = f["fb"] / F(4)
    assert np.abs(np.diff(base, axis=1)).mean() < np.abs(np.diff(noisy, axis=1)).mean()  # (it does smooth)
    for k in (1, w // 2):
        got = _gpu_denoise(mf.roll_frame(f, k), smp)
        assert np.array_equal(bits(got), bits(np.roll(base, k, axis=1))), k


# ---------------------------------------------------------------- rt_reproject_sampler
def _gpu_reproject(case, **options):
    src, aov_a, a, aov_b, b = case[:5]
    g = rt.GBuffer(a.width, a.height)
    try:
        g.upload(src[0], src[1], src[2], np.zeros(a.width * a.height, np.uint32))
        out, stats = rt.reproject_sampler(g, aov_a, a, aov_b, b, stats=True, **options)
        try:
            fb, sq, cnt, _ = out.download()
        finally:
            out.free()
    finally:
        g.free()
    return fb, sq, cnt, stats


def _host_reproject(case, **options):
    src, aov_a, a, aov_b, b = case[:5]
    return rt.reproject_sampler_host(src[0], src[1], src[2], aov_a, a, aov_b, b, stats=True, **options)


def _assert_same(got, want, what):
    for g, w_, name in zip(got[:3], want[:3], ("fb", "sq", "count")):
        a = np.ascontiguousarray(g).reshape(-1).view(np.uint32)
        b = np.ascontiguousarray(w_).reshape(-1).view(np.uint32)
        assert np.array_equal(a, b), f"{what}: {(a != b).sum()} {name} words differ; first {np.nonzero(a != b)[0][:4]}"


@pytest.mark.parametrize("shape", [(67, 45), (257, 3)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("kind", mf.KINDS)
def test_reproject_sampler_equals_host(kind, shape):
    w, h = shape
    cases = {"unmoved": mf.unmoved_case(kind, w, h, rotated=True), "moved": mf.moved_case(kind, w, h),
             "nan_position": mf.bad_camera_case(kind, w, h, "nan_position"),
             "inf_position_src": mf.bad_camera_case(kind, w, h, "inf_position_src")}
    if kind == "equirect":
        cases["yaw"] = mf.equirect_yaw_case(w, h, 7)
    if kind == "ortho":
        cases["half_pixel"] = mf.ortho_shift_case(w, h, 0.5)
    kept = {}
    for name, case in cases.items():
        got, want = _gpu_reproject(case), _host_reproject(case)
        _assert_same(got, want, f"{kind} {name}")
        assert got[3] == want[3], name
        kept[name] = got[3]["kept_pixels"]
    assert kept["nan_position"] == 0 and kept["inf_position_src"] == 0
    assert 0 < kept["moved"] < w * h and 0 < kept["unmoved"] < w * h


REAL_W, REAL_H, REAL_SPP = 96, 48, 4
REAL_MOVE = (0.04, 0.03, 0.02)  # 0.05 units and a small yaw


@pytest.mark.parametrize("kind", mf.KINDS)
def test_reproject_sampler_real_frames(kind):
    c = tq.case("room_small")
    a = scene_sampler(c, kind, REAL_W, REAL_H)
    b = scene_sampler(c, kind, REAL_W, REAL_H, move=REAL_MOVE)
    aov_a, aov_b = rt.sample_aov(c.run.dev, a), rt.sample_aov(c.run.dev, b)
    g = _sampled_gbuffer(c, a, REAL_SPP)
    try:
        src = g.download()
        out, stats = rt.reproject_sampler(g, aov_a, a, aov_b, b, stats=True)
        try:
            got = out.download()
        finally:
            out.free()
    finally:
        g.free()
    shaped = (src[0].reshape(REAL_H, REAL_W, 3), src[1].reshape(REAL_H, REAL_W), src[2].reshape(REAL_H, REAL_W))
    want = rt.reproject_sampler_host(*shaped, aov_a, a, aov_b, b, stats=True)
    _assert_same(got, want, f"{kind}: GPU vs host on room_small")
    assert stats == want[3]
    hit = int(np.isfinite(aov_b["depth"]).sum())
    print(f"{kind}: {stats['kept_pixels'] / hit:.3f} of the {hit} hit pixels kept history after the move")
    assert 0 < stats["kept_pixels"] < hit and stats["carried_samples"] == REAL_SPP * stats["kept_pixels"]
    assert np.array_equal(got[3], src[3])  # the new buffer continues the source's RNG streams


def test_reproject_sampler_writes_only_its_output():
    w, h = 67, 45
    n, pad = w * h, 192
    src, aov_a, a, aov_b, b = mf.moved_case("equirect", w, h)
    d_src = [tq.Dev(x) for x in src]
    d_a = [tq.Dev(aov_a[k]) for k in ("depth", "normal", "triangle")]
    d_b = [tq.Dev(aov_b[k]) for k in ("depth", "normal", "triangle")]
    d_out = [tq.Dev(np.full(pad + n * per + pad, FILL, np.uint32)) for per in (3, 1, 1)]
    rng = np.arange(n, dtype=np.uint32) * np.uint32(2654435761)
    d_rng = tq.Dev(rng)
    d_stats = tq.Dev(np.asarray([5, 6, 7, FILL], np.uint64))
    try:
        gs = rt.G_Buffer(d_src[0].p, d_src[1].p, d_src[2].p, d_rng.p)
        gd = rt.G_Buffer(*[d.p.value + 4 * pad for d in d_out], d_rng.p)
        rt.reproject_sampler_device(gs, [d.p for d in d_a], a, [d.p for d in d_b], b, gd, stats=d_stats.p)
        outs = [d.read() for d in d_out]
        for o in outs:
            assert (o[:pad] == FILL).all() and (o[-pad:] == FILL).all()
        want = _host_reproject((src, aov_a, a, aov_b, b))
        _assert_same([o[pad:-pad] for o in outs], want, "padded output")
        assert np.array_equal(d_rng.read(), rng)
        inputs = list(src) + [aov_a[k] for k in ("depth", "normal", "triangle")] + \
            [aov_b[k] for k in ("depth", "normal", "triangle")]
        for d, x in zip(d_src + d_a + d_b, inputs):
            assert np.array_equal(d.read().reshape(-1).view(np.uint32), np.ascontiguousarray(x).reshape(-1).view(np.uint32))
        st = [int(v) for v in d_stats.read()]
        assert st == [5 + n, 6 + want[3]["kept_pixels"], 7 + want[3]["carried_samples"], FILL]
    finally:
        for d in d_src + d_a + d_b + d_out + [d_rng, d_stats]:
            d.free()


def test_reproject_sampler_behind_chained_renders():
    """rt_reproject_sampler behind an open overlap = 1 chain joins it first: the result is that of the same calls
    unchained, the host twin's — and, for the pinhole the renderer is, rt_reproject's"""
    c = tq.case("room_small")
    w, h, P = 96, 64, 3
    a = scene_sampler(c, "pinhole", w, h)
    b = scene_sampler(c, "pinhole", w, h, move=(0.08, 0.06, 0.05))
    aov_a, aov_b = rt.sample_aov(c.run.dev, a), rt.sample_aov(c.run.dev, b)
    s = tq._stream()
    d_a = [tq.Dev(aov_a[k]) for k in ("depth", "normal", "triangle")]
    d_b = [tq.Dev(aov_b[k]) for k in ("depth", "normal", "triangle")]

    def frame(chained, samplers=True):
        g, out = rt.GBuffer(w, h), rt.GBuffer(w, h)
        try:
            for k in range(2):
                opt = rt.options(w, h, P, adaptive=False, kernel=rt.KERNEL_WAVEFRONT, overlap=chained, stream=s.value,
                                 max_depth=DEPTH)
                rt.render(c.run.dev, g, a.camera, 0 if k == 0 else 1, opt)
            if not chained:
                assert tq._HIP.hipStreamSynchronize(s) == 0
            if samplers:
                rt.reproject_sampler_device(g.g, [d.p for d in d_a], a, [d.p for d in d_b], b, out.g, stream=s.value)
            else:
                rt.reproject_device(g.g, [d.p for d in d_a], a.camera, [d.p for d in d_b], b.camera, w, h, out.g,
                                    stream=s.value)
            assert tq._HIP.hipStreamSynchronize(s) == 0
            rt.join()
            return g.download(), out.download()
        finally:
            g.free()
            out.free()

    try:
        src_plain, plain = frame(False)
        src_chained, chained = frame(True)
        _, pinhole = frame(False, samplers=False)
    finally:
        for d in d_a + d_b:
            d.free()
        assert tq._HIP.hipStreamDestroy(s) == 0
    helpers.assert_bitwise(src_chained, src_plain, what="chained source frame")
    assert int(src_plain[2].sum()) == w * h * P * 2
    _assert_same(chained, plain, "rt_reproject_sampler behind a chain")
    _assert_same(chained, pinhole, "two PINHOLE samplers vs rt_reproject")
    shaped = (src_plain[0].reshape(h, w, 3), src_plain[1].reshape(h, w), src_plain[2].reshape(h, w))
    _assert_same(chained, rt.reproject_sampler_host(*shaped, aov_a, a, aov_b, b), "chained vs host")
    assert (chained[2] == 2 * P).any() and (chained[2] == 0).any()


# ---------------------------------------------------------------- end to end
def test_panorama_history_lowers_the_error():
    """EQUIRECT 64 x 32: 16 spp at camera A, a move, the history carried by rt_reproject_sampler, 4 more spp with
    rt_sample_paths(accumulate = 1) on the carried G_Buffer — against 4 spp from a reset on the same RNG states.
    The mean absolute error against 512 spp at camera B must be the lower one: two measured errors, no threshold."""
    c = tq.case("room_small")
    w, h = 64, 32
    n = w * h
    a = scene_sampler(c, "equirect", w, h)
    b = scene_sampler(c, "equirect", w, h, move=REAL_MOVE)
    aov_a, aov_b = rt.sample_aov(c.run.dev, a), rt.sample_aov(c.run.dev, b)
    g = _sampled_gbuffer(c, a, 16)
    carried, stats = rt.reproject_sampler(g, aov_a, a, aov_b, b, stats=True)
    rng = g.download()[3]
    g.free()
    reset = rt.GBuffer(w, h)
    reset.upload(np.zeros((n, 3), F), np.zeros(n, F), np.zeros(n, np.int32), rng)
    truth = rt.GBuffer(w, h, seed_skip=5 * n)
    try:
        _sampled_gbuffer(c, b, 4, carried, accumulate=True)
        _sampled_gbuffer(c, b, 4, reset)
        _sampled_gbuffer(c, b, 512, truth)
        cfb, _, ccnt, crng = carried.download()
        rfb, _, rcnt, rrng = reset.download()
        tfb, _, tcnt, _ = truth.download()
    finally:
        for x in (carried, reset, truth):
            x.free()
    assert (tcnt == 512).all() and (rcnt == 4).all() and ccnt.min() == 4 and ccnt.max() == 20
    assert np.array_equal(crng, rrng)  # the same seeds drew the same 4 samples on both sides
    ref = tfb.astype(np.float64) / 512
    e_carried = float(np.abs(cfb.astype(np.float64) / ccnt[:, None] - ref).mean())
    e_reset = float(np.abs(rfb.astype(np.float64) / 4 - ref).mean())
    print(f"MAE carried {e_carried:.6g} reset {e_reset:.6g} ratio {e_carried / e_reset:.3f}; "
          f"{stats['kept_pixels'] / n:.3f} of the pixels kept history, mean count {ccnt.mean():.2f}")
    assert e_carried < e_reset
