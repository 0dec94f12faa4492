"""AOVs, denoising and reprojection for every camera model (rt_sample_aov, rt_denoise_sampler,
rt_reproject_sampler; include/isaklm_rt.h "frames of every camera model") without a GPU: rt_atan2f against the
C library, and the host twins — which compile the text the kernels compile — checked for the properties the
header states: the pinhole and the clamped kinds are the existing calls bit for bit, an equirectangular frame's
filter and reprojection commute with a roll of its columns, an unmoved camera of any model returns the frame.
The kernels are compared with the twins in tests/test_gpu_model_frames.py."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import denoise_ref as dref
import model_frames_ref as mf
import reproject_ref as rref
import rt

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
F = np.float32
bits = mf.bits
E_INVALID = -1


# ---------------------------------------------------------------- rt_atan2f
def test_atan2_within_one_ulp_of_the_c_library(tmp_path):
    """tests/native/atan2_check.c: 5.9 million inputs (the quadrants, the axes, ratios 2^-40 .. 2^40, the EQUIRECT
    projection's own arguments), every result within 1 float ulp of (float)atan2((double)y, (double)x), zeros,
    infinities and NaNs as C's atan2.  Measured: 0 results differ at all."""
    exe = str(tmp_path / "atan2_check")
    subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-I",
                    os.path.join(ROOT, "isaklm-raytracer_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "atan2_check.c"), "-o", exe, "-lm"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    m = re.search(r"checked (\d+) mismatches (\d+) max_ulp (\d+) special_failures (\d+)", r.stdout)
    assert m, r.stdout + r.stderr
    checked, mismatches, max_ulp, special = (int(v) for v in m.groups())
    assert checked > 5_000_000 and max_ulp <= 1 and special == 0 and r.returncode == 0, r.stdout
    assert mismatches <= checked // 1000  # (only hard-to-round cases may differ)


# ---------------------------------------------------------------- the interface
def test_header_and_binding():
    text = open(os.path.join(ROOT, "include", "isaklm_rt.h")).read()
    assert int(re.search(r"#define RT_ABI_VERSION (\d+)", text).group(1)) == 12  # an addition within ABI 12
    assert re.search(r"^#define RT_HAS_SAMPLER_FRAMES 1$", text, re.M)
    L = rt.lib()
    for name in ("rt_sample_aov", "rt_denoise_sampler", "rt_denoise_sampler_host", "rt_reproject_sampler",
                 "rt_reproject_sampler_host"):
        assert getattr(L, name).argtypes
    assert ctypes.sizeof(rt.RtSampler) == 64 and ctypes.sizeof(rt.RtAovBuffers) == 32  # no struct grew


# ---------------------------------------------------------------- rt_denoise_sampler_host
def _dn(f, smp=None, **options):
    args = (f["fb"], f["sq"], f["count"], f["depth"], f["normal"], f["albedo"])
    return rt.denoise_host(*args, **options) if smp is None else rt.denoise_sampler_host(*args, smp, **options)


@pytest.mark.parametrize("kind", ["pinhole", "fisheye", "ortho"])
@pytest.mark.parametrize("shape", dref.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_denoise_clamped_kinds_equal_rt_denoise_host(shape, kind):
    W, H = shape
    for name, options in dref.OPTION_SETS.items():
        f, want = dref.case(W, H, name)
        got = _dn(f, mf.sampler(kind, W, H), **options)
        assert got.shape == (H, W, 3) and np.array_equal(bits(got), bits(want)), name


@pytest.mark.parametrize("shape", [(67, 45), (64, 32)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_denoise_equirect_commutes_with_a_roll(shape):
    """the wrap: EQUIRECT on the frame rolled by k columns gives the output rolled by k, bit for bit — and
    rt_denoise_host, whose taps stop at the edge, does not"""
    W, H = shape
    smp = mf.sampler("equirect", W, H)
    for options in (dict(), dict(demodulate=False, iterations=3)):
        f = dref.synthetic_frame(W, H)
        base = _dn(f, smp, **options)
        clamped = _dn(f, **options)
        assert np.isfinite(base).all() and not np.array_equal(bits(base), bits(clamped))
        inner = slice(W // 2 - 2, W // 2 + 2)  # far from the seam the first level sees the same taps
        one = dict(options, iterations=1)
        assert np.array_equal(bits(_dn(f, smp, **one))[:, inner], bits(_dn(f, **one))[:, inner])
        for k in (1, W // 2, W - 1):
            rolled = mf.roll_frame(f, k)
            got = _dn(rolled, smp, **options)
            assert np.array_equal(bits(got), bits(np.roll(base, k, axis=1))), (k, options)
            assert not np.array_equal(bits(_dn(rolled, **options)), bits(np.roll(clamped, k, axis=1))), k


@pytest.mark.parametrize("shape", [(5, 4), (1, 7), (2, 3)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_denoise_equirect_tap_aliasing(shape):
    """2 * step >= width: taps alias pixels and are taken again; the roll still commutes, nothing leaves the frame"""
    W, H = shape
    smp = mf.sampler("equirect", W, H)
    f = dref.synthetic_frame(W, H)
    base = _dn(f, smp, iterations=5)
    assert base.shape == (H, W, 3) and np.isfinite(base).all()
    for k in range(1, W):
        assert np.array_equal(bits(_dn(mf.roll_frame(f, k), smp, iterations=5)), bits(np.roll(base, k, axis=1))), k
    if W == 1:  # every x neighbour is the pixel itself: the slope along x is 0, the taps repeat the column
        assert np.isfinite(_dn(f, smp, iterations=8)).all()


def test_denoise_sampler_host_errors():
    L = rt.lib()
    W, H = 6, 4
    f = dref.synthetic_frame(W, H)
    out = np.zeros((H, W, 3), F)
    p = [np.ascontiguousarray(f[k]).ctypes.data for k in ("fb", "sq", "count", "depth", "normal", "albedo")]

    def call(smp, args=p, o=None):
        return L.rt_denoise_sampler_host(*args, None if smp is None else ctypes.byref(smp), out.ctypes.data,
                                         None if o is None else ctypes.byref(o))
    good = mf.sampler("equirect", W, H).struct()
    assert call(good) == 0
    assert call(None) == E_INVALID and b"null sampler" in L.rt_last_error()
    pix = np.arange(W * H, dtype=np.int32)
    assert call(mf.sampler("equirect", W, H).struct(pix.ctypes.data)) == E_INVALID and b"pixel list" in L.rt_last_error()
    pts = np.zeros((W * H, 6), F)
    assert call(rt.Sampler("hemisphere", points=pts).struct(None, pts.ctypes.data)) == E_INVALID
    assert call(rt.RtSampler(5, W, H, rt.Camera(), 0.0, None, None)) == E_INVALID
    assert call(mf.sampler("equirect", 0, H).struct()) == E_INVALID
    assert call(mf.sampler("ortho", W, H, ortho_half_width=0.0).struct()) == E_INVALID
    assert call(mf.sampler("fisheye", W, H, fov=7.0).struct()) == E_INVALID
    for i in range(5):
        bad = list(p)
        bad[i] = None
        assert call(good, bad) == E_INVALID, i
    assert call(good, o=rt.denoise_options(iterations=9)) == E_INVALID
    with pytest.raises(ValueError):
        _dn(f, mf.sampler("equirect", W + 1, H))
    with pytest.raises(rt.RtError):
        _dn(f, mf.sampler("equirect", W, H, pixels=pix))


# ---------------------------------------------------------------- rt_reproject_sampler_host
def _rp(case, **options):
    src, aov_a, a, aov_b, b = case[:5]
    return rt.reproject_sampler_host(src[0], src[1], src[2], aov_a, a, aov_b, b, stats=True, **options)


def _same(got, want):
    for g, w, name in zip(got[:3], want[:3], ("fb", "sq", "count")):
        w = np.asarray(w).reshape(g.shape)
        bad = np.argwhere(g.view(np.uint32) != w.view(np.uint32))
        assert len(bad) == 0, f"{len(bad)} {name} values differ; first {bad[:4].tolist()}"


@pytest.mark.parametrize("name", rref.CASES)
@pytest.mark.parametrize("shape", rref.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_reproject_pinhole_equals_rt_reproject_host(shape, name):
    W, H = shape
    src, aov_a, cam_a, aov_b, cam_b, opts = rref.case(name, W, H)
    want = rt.reproject_host(src[0], src[1], src[2], aov_a, cam_a, aov_b, cam_b, stats=True, **opts)
    cam_a2 = rt.Camera(cam_a.position, cam_a.yaw, cam_a.pitch, cam_a.FOV, 0.25)  # (the aperture is ignored)
    a, b = rt.Sampler("pinhole", W, H, cam_a2), rt.Sampler("pinhole", W, H, cam_b)
    got = rt.reproject_sampler_host(src[0], src[1], src[2], aov_a, a, aov_b, b, stats=True, **opts)
    _same(got, want)
    assert got[3] == want[3]


UNMOVED = [(kind, shape, rotated, fov) for kind in mf.KINDS for shape in ((64, 32), (67, 45), (257, 129))
           for rotated in (False, True) for fov in ((3.0, 5.5) if kind == "fisheye" else (None,))]


@pytest.mark.parametrize("kind,shape,rotated,fov", UNMOVED,
                         ids=[f"{k}-{s[0]}x{s[1]}-{'rotated' if r else 'plain'}-{f}" for k, s, r, f in UNMOVED])
def test_reproject_unmoved_camera_returns_the_frame(kind, shape, rotated, fov):
    W, H = shape
    for depth in (0.37, 4.0, 55.0, None):  # (None: a depth of its own per pixel)
        case = mf.unmoved_case(kind, W, H, depth, rotated, fov)
        src, aov = case[0], case[3]
        fb, sq, cnt, st = _rp(case, max_history=64)
        hit = np.isfinite(aov["depth"]) & (src[2] > 0)
        assert hit.sum() > W * H // 5
        assert np.array_equal(cnt[hit], src[2][hit]), (depth, int((cnt[hit] != src[2][hit]).sum()))
        assert np.array_equal(bits(fb)[hit], bits(src[0])[hit]) and np.array_equal(bits(sq)[hit], bits(src[1])[hit])
        assert (cnt[~hit] == 0).all() and (bits(fb)[~hit] == 0).all() and (bits(sq)[~hit] == 0).all()
        assert st["kept_pixels"] == int(hit.sum())
    if kind == "fisheye":  # the pixels outside the image circle have no ray: they are among the resets
        assert (~mf.in_frame(case[2])).sum() > 0


@pytest.mark.parametrize("k", [1, 7])
@pytest.mark.parametrize("shape", [(64, 32), (67, 45)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_reproject_equirect_yaw_rolls_the_frame(shape, k):
    W, H = shape
    case = mf.equirect_yaw_case(W, H, k)
    src, shift = case[0], case[5]
    assert shift in (k, W - k)
    fb, sq, cnt, _ = _rp(case)
    want = [np.roll(a, -shift, axis=1) for a in src]
    hit = np.isfinite(case[3]["depth"]) & (want[2] > 0)
    assert hit[:, :k + 1].any() and hit[:, -k - 1:].any()  # (pixels on both sides of the seam carry history)
    for got, w in zip((fb, sq, cnt), want):
        assert np.array_equal(got.view(np.uint32)[hit], w.view(np.uint32)[hit])
        assert not got[~hit].any()


def test_reproject_ortho_shift_moves_the_frame():
    W, H, k = 64, 32, 3
    case = mf.ortho_shift_case(W, H, k)
    src = case[0]
    fb, sq, cnt, st = _rp(case)
    assert np.array_equal(cnt[:, :W - k], src[2][:, k:]) and (cnt[:, W - k:] == 0).all()
    assert np.array_equal(bits(fb)[:, :W - k], bits(src[0])[:, k:]) and (bits(fb)[:, W - k:] == 0).all()
    assert np.array_equal(bits(sq)[:, :W - k], bits(src[1])[:, k:]) and (bits(sq)[:, W - k:] == 0).all()
    assert st["kept_pixels"] == (W - k) * H
    # a plane 10 % nearer than the source's guides say: past the 2 % tolerance on z_exp = c.z
    aov_b = {n: v.copy() for n, v in case[3].items()}
    aov_b["depth"] *= F(0.9)
    assert _rp((src, case[1], case[2], aov_b, case[4]))[3]["kept_pixels"] == 0


def _half_shift_check(case, fb, cnt, col_counts, wrap):
    src = case[0]
    H, W = cnt.shape
    nxt = np.roll(col_counts, -1)
    want = np.minimum(col_counts, nxt)
    cols = slice(0, W) if wrap else slice(0, W - 1)
    assert np.array_equal(cnt[:, cols], np.broadcast_to(want[cols], (H, want[cols].size)))
    m = src[0].astype(np.float64) / src[2][..., None]
    m2 = np.roll(m, -1, axis=1)
    mid, span = 0.5 * (m + m2), np.abs(m - m2)
    got_mean = fb[:, cols].astype(np.float64) / cnt[:, cols, None]
    # the two neighbours' average: weights 1/2 within the projection's error (5e-4 pixel), as the pinhole's plane
    assert (np.abs(got_mean - mid[:, cols]) <= 2e-3 * span[:, cols] + 1e-5).all()


def test_reproject_half_pixel_shift_takes_four_taps():
    W, H = 64, 32
    col_counts = np.asarray([3 + (7 * x) % 11 for x in range(W)], np.int32)  # neighbours differ
    case = mf.ortho_shift_case(W, H, 0.5, counts=col_counts[None, :])
    fb, sq, cnt, _ = _rp(case)
    _half_shift_check(case, fb, cnt, col_counts, wrap=False)
    # EQUIRECT: half a column of yaw, the same surface everywhere; the seam's pixels blend columns W - 1 and 0
    a = mf.sampler("equirect", W, H)
    b = mf.sampler("equirect", W, H, yaw=float(F(0.5) * mf.yaw_step(W)))
    if mf.column_shift(a, mf.sampler("equirect", W, H, yaw=float(mf.yaw_step(W)))) != 1:
        b = mf.sampler("equirect", W, H, yaw=float(F(-0.5) * mf.yaw_step(W)))
    nrm = np.zeros((H, W, 3), F)
    nrm[..., 1] = 1
    aov = dict(depth=np.full((H, W), 4.0, F), normal=nrm, triangle=np.full((H, W), 5, np.int32))
    fb0, sq0, count = rref.sums(W, H, 5, counts=(1, 2, 7, 20, 64))
    count2 = np.broadcast_to(col_counts, (H, W)).copy()
    src = ((fb0 / count[..., None].astype(F) * count2[..., None].astype(F)).astype(F), sq0, count2)
    case = (src, aov, a, aov, b)
    fb, sq, cnt, st = _rp(case)
    assert st["kept_pixels"] == W * H
    _half_shift_check(case, fb, cnt, col_counts, wrap=True)


@pytest.mark.parametrize("kind", mf.KINDS)
def test_reproject_bad_cameras_reset_every_pixel(kind):
    L = rt.lib()
    W, H = 67, 45
    n, pad = W * H, 256
    for name in mf.BAD_CAMERAS:
        src, aov_a, a, aov_b, b = mf.bad_camera_case(kind, W, H, name)
        arrs = [np.ascontiguousarray(x) for x in (src[0], src[1], src[2], aov_a["depth"], aov_a["normal"],
                                                  aov_a["triangle"], aov_b["depth"], aov_b["normal"], aov_b["triangle"])]
        outs = [np.full(pad + n * per + pad, 0x5A5A5A5A, np.uint32) for per in (3, 1, 1)]
        st = np.zeros(3, np.uint64)
        p = [x.ctypes.data for x in arrs]
        rc = L.rt_reproject_sampler_host(*p[:6], ctypes.byref(a.struct()), *p[6:], ctypes.byref(b.struct()),
                                         *[o.ctypes.data + 4 * pad for o in outs], st.ctypes.data, None)
        assert rc == 0, name
        for o in outs:
            assert (o[:pad] == 0x5A5A5A5A).all() and (o[-pad:] == 0x5A5A5A5A).all(), name
            assert not o[pad:-pad].any(), (kind, name, int(np.count_nonzero(o[pad:-pad])))
        assert st.tolist() == [n, 0, 0], name


def test_reproject_nan_guides_stay_in_bounds():
    """NaN, -inf and negative depths on the new side: each pixel resets or keeps finite sums"""
    for kind in mf.KINDS:
        src, aov_a, a, aov_b, b = mf.unmoved_case(kind, 67, 45)
        rs = np.random.RandomState(13)
        r = rs.uniform(size=aov_b["depth"].shape)
        z = np.where(r < 0.2, F(np.nan), np.where(r < 0.4, -mf.INF, np.where(r < 0.5, F(-3.0), aov_b["depth"]))).astype(F)
        fb, sq, cnt, st = _rp((src, aov_a, a, dict(aov_b, depth=z), b))
        assert np.isfinite(fb).all() and np.isfinite(sq).all() and (cnt >= 0).all() and (cnt <= 64).all()
        assert (cnt[~(z < mf.INF)] == 0).all() and 0 < st["kept_pixels"] < 67 * 45


def test_reproject_sampler_host_errors():
    L = rt.lib()
    W, H = 6, 4
    src, aov_a, a, aov_b, b = mf.unmoved_case("equirect", W, H)
    arrs = [np.ascontiguousarray(x) for x in (src[0], src[1], src[2], aov_a["depth"], aov_a["normal"],
                                              aov_a["triangle"], aov_b["depth"], aov_b["normal"], aov_b["triangle"])]
    outs = [np.zeros((H, W, 3), F), np.zeros((H, W), F), np.zeros((H, W), np.int32)]
    st = np.zeros(3, np.uint64)
    p = [x.ctypes.data for x in arrs]
    q = [x.ctypes.data for x in outs]
    sa, sb = a.struct(), b.struct()

    def call(p=p, q=q, sa=sa, sb=sb, o=None):
        return L.rt_reproject_sampler_host(*p[:6], None if sa is None else ctypes.byref(sa), *p[6:],
                                           None if sb is None else ctypes.byref(sb), *q, st.ctypes.data,
                                           None if o is None else ctypes.byref(o))
    assert call() == 0
    assert call(sa=None) == E_INVALID and call(sb=None) == E_INVALID
    assert call(sb=mf.sampler("fisheye", W, H).struct()) == E_INVALID and b"differ" in L.rt_last_error()
    assert call(sa=mf.sampler("equirect", W + 1, H).struct()) == E_INVALID
    assert call(sb=mf.sampler("equirect", W, H + 1).struct()) == E_INVALID
    pix = np.arange(W * H, dtype=np.int32)
    assert call(sa=a.struct(pix.ctypes.data)) == E_INVALID and b"pixel list" in L.rt_last_error()
    assert call(sb=b.struct(pix.ctypes.data)) == E_INVALID
    pts = np.zeros((W * H, 6), F)
    hemi = rt.Sampler("hemisphere", points=pts).struct(None, pts.ctypes.data)
    assert call(sa=hemi, sb=hemi) == E_INVALID
    assert call(sa=rt.RtSampler(5, W, H, rt.Camera(), 0.0, None, None), sb=rt.RtSampler(5, W, H, rt.Camera(), 0.0, None, None)) == E_INVALID
    for i in range(9):
        bad = list(p)
        bad[i] = None
        assert call(p=bad) == (0 if i in (5, 8) else E_INVALID), i  # (the triangle buffers are optional)
    for i in range(3):
        bad = list(q)
        bad[i] = None
        assert call(q=bad) == E_INVALID, i
    assert call(q=[p[0], q[1], q[2]]) == E_INVALID and b"overlap" in L.rt_last_error()
    assert call(q=[q[0], p[1] + 4, q[2]]) == E_INVALID
    assert call(q=[q[0], q[1], p[2] + 4 * (W * H - 1)]) == E_INVALID
    assert call(o=rt.reproject_options(max_history=-1)) == E_INVALID
    assert call(o=rt.reproject_options(depth_tol=float("nan"))) == E_INVALID
    with pytest.raises(rt.RtError):
        rt.reproject_sampler_host(src[0], src[1], src[2], aov_a, mf.sampler("ortho", W, H), aov_b, b)
    with pytest.raises(ValueError):
        rt.reproject_sampler_host(src[0], src[1], src[2], aov_a, a, aov_b, mf.sampler("equirect", W + 1, H))


def test_device_calls_reject_bad_arguments_without_a_device():
    """rt_sample_aov, rt_denoise_sampler and rt_reproject_sampler refuse these before any GPU call: the pointers
    below are not device memory and the scene is never looked at"""
    L = rt.lib()
    W, H = 8, 8
    a, b = 0x100000, 0x900000
    gs = rt.G_Buffer(a, a + 0x10000, a + 0x20000, a + 0x30000)
    gd = rt.G_Buffer(b, b + 0x10000, b + 0x20000, a + 0x30000)
    aov = rt.RtAovBuffers(0x2000, 0x3000, 0x4000, None)
    eq = mf.sampler("equirect", W, H)
    pts = 0x8000
    hemi = rt.RtSampler(rt.SAMPLER_HEMISPHERE, 0, 0, rt.Camera(), 0.0, None, pts)
    listed = eq.struct(0x5000)

    def dn(smp, g=gs, aov=aov, out=0x6000, o=None):
        return L.rt_denoise_sampler(g, None if aov is None else ctypes.byref(aov), None if smp is None else ctypes.byref(smp),
                                    out, None if o is None else ctypes.byref(o))
    for smp in (None, hemi, listed, mf.sampler("equirect", 0, H).struct(), mf.sampler("fisheye", W, H, fov=0.0).struct()):
        assert dn(smp) == E_INVALID
    assert dn(eq.struct(), aov=None) == E_INVALID and dn(eq.struct(), out=None) == E_INVALID
    assert dn(eq.struct(), out=0x6002) == E_INVALID and dn(eq.struct(), o=rt.denoise_options(iterations=9)) == E_INVALID

    def rp(sa, sb, gs=gs, gd=gd, o=None):
        return L.rt_reproject_sampler(gs, ctypes.byref(aov), None if sa is None else ctypes.byref(sa), ctypes.byref(aov),
                                      None if sb is None else ctypes.byref(sb), gd, None if o is None else ctypes.byref(o))
    good = eq.struct()
    assert rp(None, good) == E_INVALID and rp(good, None) == E_INVALID
    assert rp(good, mf.sampler("ortho", W, H).struct()) == E_INVALID
    assert rp(good, mf.sampler("equirect", W, H + 1).struct()) == E_INVALID
    assert rp(listed, good) == E_INVALID and rp(good, listed) == E_INVALID and rp(hemi, hemi) == E_INVALID
    assert rp(good, good, gd=rt.G_Buffer(a, b + 0x10000, b + 0x20000, None)) == E_INVALID  # dst fb = src fb
    assert rp(good, good, gs=rt.G_Buffer(None, a + 0x10000, a + 0x20000, None)) == E_INVALID
    assert rp(good, good, o=rt.reproject_options(normal_min=1.5)) == E_INVALID

    def aovs(smp, n, bufs=aov):
        return L.rt_sample_aov(None, None if smp is None else ctypes.byref(smp), n, None if bufs is None else ctypes.byref(bufs), None)
    assert aovs(good, W * H, None) == E_INVALID and b"null buffers" in L.rt_last_error()
    assert aovs(good, W * H, rt.RtAovBuffers(0x2002, None, None, None)) == E_INVALID
    assert aovs(None, W * H) == E_INVALID and aovs(good, W * H - 1) == E_INVALID and aovs(good, -1) == E_INVALID
    assert aovs(hemi, 4) == E_INVALID and b"hemisphere" in L.rt_last_error()
    assert aovs(eq.struct(0x5002), 4) == E_INVALID
    assert aovs(good, W * H) == E_INVALID and b"null scene" in L.rt_last_error()  # (the sampler itself passed)
