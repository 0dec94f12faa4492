"""rt_denoise on the GPU (csrc/denoise.hip): bit-identical to rt_denoise_host
and to the numpy restatement (tests/denoise_ref.py) on the synthetic frames
of tests/test_denoise_cpu.py and on a real 4-spp frame; writes nothing past
its output; lowers the error of a low-spp frame against a 1024-spp reference;
joins chained renders as rt_tonemap does; rt_tonemap_rgb and the driver's
--denoise."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

import denoise_ref
import helpers
import rt

pytestmark = pytest.mark.gpu
F = np.float32
bits = denoise_ref.bits

_HIP = None


def _stream():
    global _HIP
    if _HIP is None:
        _HIP = ctypes.CDLL("libamdhip64.so")
    s = ctypes.c_void_p()
    assert _HIP.hipStreamCreate(ctypes.byref(s)) == 0
    return s


def _gbuffer(f):
    """the synthetic frame in a rt_gbuffer_create buffer (rt_upload)"""
    H, W = f["depth"].shape
    g = rt.GBuffer(W, H)
    g.upload(f["fb"], f["sq"], f["count"], np.zeros(W * H, np.uint32))
    return g


def _assert_same_bits(a, b, what):
    bad = np.argwhere(bits(a) != bits(b))
    assert len(bad) == 0, f"{what}: {len(bad)} of {a.size} values differ; first (y, x, c) {bad[:4].tolist()}: " \
                          f"{[float(a[tuple(i)]) for i in bad[:4]]} vs {[float(b[tuple(i)]) for i in bad[:4]]}"


def _host(f, **options):
    return rt.denoise_host(f["fb"], f["sq"], f["count"], f["depth"], f["normal"], f["albedo"], **options)


# ---------------------------------------------------------------- synthetic frames, bit for bit
@pytest.mark.parametrize("name", list(denoise_ref.OPTION_SETS))
@pytest.mark.parametrize("shape", denoise_ref.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_gpu_equals_host_and_restatement(shape, name):
    W, H = shape
    f, ref = denoise_ref.case(W, H, name)
    options = denoise_ref.OPTION_SETS[name]
    g = _gbuffer(f)
    try:
        out = rt.denoise(g, f, **options)
    finally:
        g.free()
    assert out.shape == (H, W, 3)
    _assert_same_bits(out, _host(f, **options), "GPU vs host")
    _assert_same_bits(out, ref, "GPU vs restatement")


@pytest.mark.parametrize("name", ["defaults", "iterations8"])
def test_partial_last_block_and_row_phases(name):
    """257 x 3: the ninth 32-pixel tile of a row holds one pixel, the tile rows above the third are empty, and
    the three rows start at 16-byte phases 0, 4 and 8 of the 12-byte output records"""
    W, H = 257, 3
    f = denoise_ref.synthetic_frame(W, H)
    options = denoise_ref.OPTION_SETS[name]
    g = _gbuffer(f)
    try:
        out = rt.denoise(g, f, **options)
    finally:
        g.free()
    _assert_same_bits(out, _host(f, **options), "GPU vs host")
    ref = denoise_ref.denoise(f["fb"], f["sq"], f["count"], f["depth"], f["normal"], f["albedo"], **options)
    _assert_same_bits(out, ref, "GPU vs restatement")


def test_stream_and_untouched_tail():
    """on a non-null stream, into a padded, pre-filled output: the slots beyond width*height*3 keep their fill;
    then a frame of another size (the workspace is replaced) and the first size again"""
    s = _stream()
    try:
        for W, H in ((37, 29), (64, 48), (37, 29)):
            f, ref = denoise_ref.case(W, H, "defaults")
            n = W * H
            g = _gbuffer(f)
            fill = np.full(3 * n + 67, np.float32(-7.25))
            d_out, d_depth, d_normal, d_albedo = (rt.DeviceArray(x) for x in (fill, f["depth"], f["normal"], f["albedo"]))
            try:
                rt.denoise_device(g.g, (d_depth.p, d_normal.p, d_albedo.p), W, H, d_out.p, stream=s.value)
                assert _HIP.hipStreamSynchronize(s) == 0
                got = d_out.read()
            finally:
                for d in (d_out, d_depth, d_normal, d_albedo):
                    d.free()
                g.free()
            _assert_same_bits(got[:3 * n].reshape(H, W, 3), ref, f"stream {W}x{H}")
            assert (got[3 * n:] == np.float32(-7.25)).all()
    finally:
        assert _HIP.hipStreamDestroy(s) == 0


def test_two_sizes_on_two_streams_equal_alone():
    """two calls of different frame sizes on two streams, issued back to back with nothing between them: the
    second replaces the device's workspace while the first may still be using it, so the library waits for the
    first before it frees the buffers.  Each output is the one of the same call made alone."""
    shapes = ((96, 64), (64, 48))
    streams = [_stream(), _stream()]
    frames = [denoise_ref.case(W, H, "defaults") for W, H in shapes]
    gs = [_gbuffer(f) for f, _ in frames]
    devs = [[rt.DeviceArray(f[k]) for k in ("depth", "normal", "albedo")] for f, _ in frames]
    outs = [rt.DeviceArray(np.zeros(3 * W * H, F)) for W, H in shapes]
    try:
        for (W, H), g, (d_depth, d_normal, d_albedo), d_out, s in zip(shapes, gs, devs, outs, streams):
            rt.denoise_device(g.g, (d_depth.p, d_normal.p, d_albedo.p), W, H, d_out.p, stream=s.value)
        for s in streams:
            assert _HIP.hipStreamSynchronize(s) == 0
        got = [d.read() for d in outs]
        alone = [rt.denoise(g, f) for g, (f, _) in zip(gs, frames)]
    finally:
        for d in outs + [d for ds in devs for d in ds]:
            d.free()
        for g in gs:
            g.free()
        for s in streams:
            assert _HIP.hipStreamDestroy(s) == 0
    for (W, H), out, one, (_, ref) in zip(shapes, got, alone, frames):
        _assert_same_bits(out.reshape(H, W, 3), one, f"{W}x{H} on its stream vs alone")
        _assert_same_bits(one, ref, f"{W}x{H} alone vs restatement")


# ---------------------------------------------------------------- a real frame
W_REAL, H_REAL, SPP, DEPTH = 96, 64, 4, 8
# relMSE(denoised 4 spp) / relMSE(raw 4 spp) measured on the MI355X (DESIGN.md "Denoising"; renders are
# bit-reproducible, so it is one number for a given tree), times 1.25: a change to the filter's constants that
# costs more than that has to show itself.  Below 1 whatever the measurement: a denoiser that raises the error
# has failed.
MEASURED_RATIO = 0.291663  # relMSE raw 1.31598, denoised 0.383822
RATIO_BOUND = min(MEASURED_RATIO * 1.25, 0.999)


@pytest.fixture(scope="module")
def room():
    run = helpers.GpuRun("room_small")
    gpu, _, g = run.render(W_REAL, H_REAL, SPP, adaptive=False, max_depth=DEPTH)
    aov = rt.render_aov(run.dev, run.camera, W_REAL, H_REAL)
    yield run, gpu, g, aov
    g.free()


def test_real_frame_equals_host(room):
    run, (fb, sq, cnt, _), g, aov = room
    out = rt.denoise(g, aov)
    host = rt.denoise_host(fb, sq, cnt, aov["depth"], aov["normal"], aov["albedo"])
    assert np.isfinite(out).all()
    _assert_same_bits(out, host, "GPU vs host on room_small")
    plain = rt.denoise(g, aov, demodulate=False)
    _assert_same_bits(plain, rt.denoise_host(fb, sq, cnt, aov["depth"], aov["normal"], None, demodulate=False),
                      "GPU vs host, no demodulation")
    assert (bits(out) != bits(plain)).any()


def _rel_mse(a, ref):
    a, ref = a.astype(np.float64).reshape(-1, 3), ref.astype(np.float64).reshape(-1, 3)
    return float(np.mean((a - ref) ** 2 / (ref ** 2 + 0.01)))


def test_noise_drops(room):
    """relMSE against the same scene at 1024 spp (6.3 M samples): the denoised 4-spp frame is closer to it than
    the raw one"""
    run, (fb, _, cnt, _), g, aov = room
    (rfb, _, rcnt, _), _, rg = run.render(W_REAL, H_REAL, 256, calls=4, adaptive=False, max_depth=DEPTH)
    rg.free()
    assert (rcnt == 1024).all() and (cnt == SPP).all()
    ref = rfb / rcnt[:, None]
    raw = fb / cnt[:, None]
    den = rt.denoise(g, aov)
    e_raw, e_den = _rel_mse(raw, ref), _rel_mse(den, ref)
    print(f"relMSE raw {e_raw:.6g} denoised {e_den:.6g} ratio {e_den / e_raw:.6g}")
    assert e_den < e_raw
    assert e_den / e_raw < RATIO_BOUND


def test_tonemap_rgb_matches_tonemap(room):
    _, (fb, _, cnt, _), g, _ = room
    mean = (fb * (F(1) / cnt.astype(F))[:, None]).astype(F).reshape(H_REAL, W_REAL, 3)
    a = rt.tonemap(g)
    b = rt.tonemap_rgb(mean)
    assert a.shape == b.shape == (W_REAL * H_REAL, 4)
    assert np.max(np.abs(a.astype(int) - b.astype(int))) <= 1
    assert (b[:, 3] == 255).all()


# ---------------------------------------------------------------- chained renders
@pytest.mark.parametrize("coalesce", [-1, 0])
def test_denoise_between_chained_renders(room, coalesce):
    """rt_denoise between two chained rt_render calls (overlap = 1) sees the completed frame — its result is the
    one after an explicit rt_join — and the continued render is the uninterrupted one: rt_tonemap's contract"""
    run, _, _, aov = room
    W, H, P = W_REAL, H_REAL, 3
    n = W * H
    s = _stream()
    d_depth, d_normal, d_albedo = (rt.DeviceArray(aov[k]) for k in ("depth", "normal", "albedo"))

    def frame(mode):
        g = rt.GBuffer(W, H)
        d_out = rt.DeviceArray(np.zeros(3 * n, F))
        try:
            for k in range(3):
                opt = rt.options(W, H, P, adaptive=False, kernel=rt.KERNEL_WAVEFRONT, overlap=True,
                                 coalesce_passes=coalesce, stream=s.value)
                rt.render(run.dev, g, run.camera, 0 if k == 0 else 1, opt)
                if k == 1 and mode == "joined":
                    rt.join()
                if k == 1 and mode != "plain":
                    rt.denoise_device(g.g, (d_depth.p, d_normal.p, d_albedo.p), W, H, d_out.p, stream=s.value)
            rt.join()
            assert _HIP.hipStreamSynchronize(s) == 0
            return g.download(), d_out.read()
        finally:
            d_out.free()
            g.free()

    try:
        plain, _ = frame("plain")
        mixed, den_mixed = frame("between")
        joined, den_joined = frame("joined")
    finally:
        for d in (d_depth, d_normal, d_albedo):
            d.free()
        assert _HIP.hipStreamDestroy(s) == 0
    helpers.assert_bitwise(mixed, plain, what="chained frame with rt_denoise in between")
    helpers.assert_bitwise(joined, plain, what="chained frame with a join and rt_denoise in between")
    assert int(plain[2].sum()) == n * P * 3
    assert np.array_equal(bits(den_mixed), bits(den_joined))
    assert np.isfinite(den_mixed).all() and den_mixed.any()


# ---------------------------------------------------------------- the driver
def _png_size(path):
    with open(path, "rb") as fh:
        head = fh.read(24)
    assert head[:8] == b"\x89PNG\r\n\x1a\n" and head[12:16] == b"IHDR"
    return struct.unpack(">II", head[16:24])


def test_cli_denoise(tmp_path):
    exe = os.path.join(os.path.dirname(rt.LIB_PATH), "rt_render")
    W, H = 96, 64
    common = ["--width", str(W), "--height", str(H), "--spp", "4", "--quiet"]
    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir()
    b.mkdir()
    r = subprocess.run([exe, "--generate", "room_small", str(tmp_path / "scene_a")] + common +
                       ["--denoise", "--out", str(a / "x.png")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe, "--generate", "room_small", str(tmp_path / "scene_b")] + common +
                       ["--out", str(b / "x.png")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert _png_size(a / "x.denoised.png") == (W, H)
    assert not (b / "x.denoised.png").exists()
    assert (a / "x.png").read_bytes() == (b / "x.png").read_bytes()
    assert (a / "x.denoised.png").read_bytes() != (a / "x.png").read_bytes()
