"""Temporal reprojection (rt_reproject / rt_reproject_host, include/isaklm_rt.h)
without a GPU.  rt_reproject_host compiles the text the kernel compiles
(csrc/reproject_math.h); here it is compared bit for bit with the numpy
restatement of the definition (tests/reproject_ref.py), checked for properties
that do not lean on the restatement — an unmoved camera returns the frame, a
whole-pixel move shifts it, each rejection rule alone resets its pixels — and
for its argument errors.  The kernel is compared with it in
tests/test_gpu_reproject.py."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import reproject_ref as ref
import rt

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
INC = os.path.join(ROOT, "include")
E_INVALID = -1
F = np.float32
bits = ref.bits


def _host(src, aov_a, cam_a, aov_b, cam_b, **options):
    return rt.reproject_host(src[0], src[1], src[2], aov_a, cam_a, aov_b, cam_b, stats=True, **options)


def _same(got, want):
    fb, sq, cnt = got[:3]
    H, W = cnt.shape
    assert np.array_equal(cnt, np.asarray(want[2]).reshape(H, W)), \
        f"{(cnt != want[2]).sum()} counts differ; first {np.argwhere(cnt != want[2])[:4].tolist()}"
    bad = np.argwhere(bits(fb) != bits(np.asarray(want[0]).reshape(H, W, 3)))
    assert len(bad) == 0, f"{len(bad)} fb values differ; first (y, x, c) {bad[:4].tolist()}"
    bad = np.argwhere(bits(sq) != bits(np.asarray(want[1]).reshape(H, W)))
    assert len(bad) == 0, f"{len(bad)} sq values differ; first (y, x) {bad[:4].tolist()}"


# ---------------------------------------------------------------- the restatement, bit for bit
@pytest.mark.parametrize("name", ref.CASES)
@pytest.mark.parametrize("shape", ref.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_host_equals_restatement(shape, name):
    W, H = shape
    src, aov_a, cam_a, aov_b, cam_b, opts = ref.case(name, W, H)
    got = _host(src, aov_a, cam_a, aov_b, cam_b, **opts)
    want = ref.reproject(src[0], src[1], src[2], aov_a, cam_a, aov_b, cam_b, **opts)
    assert got[0].shape == (H, W, 3) and got[1].shape == (H, W) and got[2].dtype == np.int32
    assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
    _same(got, want)
    assert got[3] == want[3]  # the stats
    assert got[3]["pixels"] == W * H and got[3]["kept_pixels"] == int((got[2] > 0).sum())
    assert got[3]["carried_samples"] == int(got[2].astype(np.int64).sum())


def test_synthetic_cases_cover_the_paths():
    """the shared cases are not trivially all-reset or all-kept, and take both tap modes"""
    W, H = 64, 48
    kept = {}
    for name in ref.CASES:
        src, aov_a, cam_a, aov_b, cam_b, opts = ref.case(name, W, H)
        kept[name] = _host(src, aov_a, cam_a, aov_b, cam_b, **opts)[3]["kept_pixels"] / (W * H)
    assert kept["unmoved"] > 0.5 and kept["far_unmoved"] > 0.5
    assert 0.2 < kept["small_move"] < 0.95 and 0.05 < kept["dolly_in"] < 0.95
    assert 0.0 < kept["tight_options"] < kept["no_triangles"]
    assert kept["large_turn"] == 0 and 0.0 < kept["behind"] < 0.3  # (the far wall is in front of both cameras)
    assert kept["nan_camera"] == 0 and kept["inf_camera"] == 0 and kept["nan_src_camera"] == 0
    assert 0.0 < kept["nan_depth"] < kept["unmoved"] and 0.0 < kept["nan_sums"] < kept["unmoved"]
    src, aov_a, cam_a, aov_b, cam_b, _ = ref.case("small_move", W, H)
    assert np.isinf(aov_b["depth"]).any() and (src[2] == 0).any()
    assert len(np.unique(aov_b["normal"].reshape(-1, 3), axis=0)) >= 3


# ---------------------------------------------------------------- an unmoved camera returns the frame
@pytest.mark.parametrize("name", ["unmoved", "far_unmoved"])
@pytest.mark.parametrize("shape", ref.SHAPES[:2], ids=lambda s: f"{s[0]}x{s[1]}")
def test_unmoved_camera_returns_the_frame(shape, name):
    W, H = shape
    src, aov_a, cam_a, aov_b, cam_b, _ = ref.case(name, W, H)
    fb, sq, cnt, _ = _host(src, aov_a, cam_a, aov_b, cam_b, max_history=1 << 20)
    hit = np.isfinite(aov_b["depth"]) & (src[2] > 0)
    assert hit.sum() > W * H // 2
    assert np.array_equal(cnt[hit], src[2][hit])
    assert np.array_equal(bits(fb)[hit], bits(src[0])[hit]) and np.array_equal(bits(sq)[hit], bits(src[1])[hit])
    assert (cnt[~hit] == 0).all() and (bits(fb)[~hit] == 0).all() and (bits(sq)[~hit] == 0).all()


def test_unmoved_camera_caps_the_history():
    W, H = 64, 48
    src, aov_a, cam_a, aov_b, cam_b, _ = ref.case("far_unmoved", W, H)
    mean = (src[0] / np.maximum(src[2], 1)[..., None].astype(F)).astype(F)
    count = np.full((H, W), 20, np.int32)
    fb = (mean * F(20)).astype(F)
    sq = (src[1] + F(1)).astype(F)
    out_fb, out_sq, cnt, _ = _host((fb, sq, count), aov_a, cam_a, aov_b, cam_b, max_history=8)
    hit = np.isfinite(aov_b["depth"])
    assert (cnt[hit] == 8).all() and (cnt[~hit] == 0).all()
    assert np.array_equal(bits(out_fb)[hit], bits((fb * (F(1) / F(20))) * F(8))[hit])
    assert np.array_equal(bits(out_sq)[hit], bits((sq / F(20)) * F(8))[hit])


# ---------------------------------------------------------------- whole- and half-pixel moves over a plane
@pytest.mark.parametrize("dist", [4.0, 0.37])
def test_exact_shift(dist):
    W, H, k = 64, 48, 3
    src, aov_a, cam_a, aov_b, cam_b = ref.plane_case(W, H, dist, shift_x=k)
    fb, sq, cnt, st = _host(src, aov_a, cam_a, aov_b, cam_b)
    assert np.array_equal(cnt[:, :W - k], src[2][:, k:]) and (cnt[:, W - k:] == 0).all()
    assert np.array_equal(bits(fb)[:, :W - k], bits(src[0])[:, k:]) and (bits(fb)[:, W - k:] == 0).all()
    assert np.array_equal(bits(sq)[:, :W - k], bits(src[1])[:, k:]) and (bits(sq)[:, W - k:] == 0).all()
    assert st["kept_pixels"] == (W - k) * H
    src, aov_a, cam_a, aov_b, cam_b = ref.plane_case(W, H, dist, shift_y=-k)
    fb, sq, cnt, _ = _host(src, aov_a, cam_a, aov_b, cam_b)
    assert np.array_equal(cnt[k:], src[2][:H - k]) and (cnt[:k] == 0).all()
    assert np.array_equal(bits(fb)[k:], bits(src[0])[:H - k]) and (bits(fb)[:k] == 0).all()
    assert np.array_equal(bits(sq)[k:], bits(src[1])[:H - k]) and (bits(sq)[:k] == 0).all()


def test_half_pixel_shift():
    W, H = 64, 48
    col_counts = np.asarray([3 + (7 * x) % 11 for x in range(W)], np.int32)  # neighbours differ
    src, aov_a, cam_a, aov_b, cam_b = ref.plane_case(W, H, 4.0, shift_x=0.5, counts=col_counts[None, :])
    got = _host(src, aov_a, cam_a, aov_b, cam_b)
    _same(got, ref.reproject(src[0], src[1], src[2], aov_a, cam_a, aov_b, cam_b))
    fb, sq, cnt, _ = got
    want = np.minimum(col_counts[:-1], col_counts[1:])
    assert np.array_equal(cnt[:, :W - 1], np.broadcast_to(want, (H, W - 1)))
    # the mean is the two neighbours' average: weights 1/2 within the projection's error (5e-4 pixel)
    m = src[0].astype(np.float64) / src[2][..., None]
    mid = 0.5 * (m[:, :-1] + m[:, 1:])
    span = np.abs(m[:, :-1] - m[:, 1:])
    inner = slice(1, H - 1)
    got_mean = fb[inner, :W - 1].astype(np.float64) / cnt[inner, :W - 1, None]
    assert (np.abs(got_mean - mid[inner]) <= 2e-3 * span[inner] + 1e-5).all()


# ---------------------------------------------------------------- the rejections, each alone
STRIP = slice(10, 15)


def _strip_case(change, **options):
    """the unmoved plane with columns STRIP of the old frame changed by `change`; -> (count, src count)"""
    W, H = 64, 48
    src, aov_a, cam_a, aov_b, cam_b = ref.plane_case(W, H, 4.0)
    src = tuple(a.copy() for a in src)
    change(src, aov_a)
    got = _host(src, aov_a, cam_a, aov_b, cam_b, **options)
    _same(got, ref.reproject(src[0], src[1], src[2], aov_a, cam_a, aov_b, cam_b, **options))
    return got[2], src[2]


def _only_strip_reset(cnt, src_cnt):
    rest = np.ones(cnt.shape[1], bool)
    rest[STRIP] = False
    return (cnt[:, STRIP] == 0).all() and np.array_equal(cnt[:, rest], src_cnt[:, rest])


def test_foreground_strip_resets():
    def nearer(src, aov):
        aov["depth"][:, STRIP] *= F(0.9)  # 10 % nearer: past the 2 % tolerance
    assert _only_strip_reset(*_strip_case(nearer))
    cnt, src_cnt = _strip_case(nearer, depth_tol=0.15)
    assert np.array_equal(cnt, src_cnt)

    def slightly(src, aov):
        aov["depth"][:, STRIP] *= F(0.99)
    cnt, src_cnt = _strip_case(slightly)
    assert np.array_equal(cnt, src_cnt)


def test_turned_normal_resets():
    def turn(src, aov):
        aov["normal"][:, STRIP] = np.asarray([0.6, 0.0, -0.8], F)  # cos 0.8 < 0.95
    assert _only_strip_reset(*_strip_case(turn))
    cnt, src_cnt = _strip_case(turn, normal_min=0.75)
    assert np.array_equal(cnt, src_cnt)


def test_other_triangle_resets_only_when_matching():
    def other(src, aov):
        aov["triangle"][:, STRIP] = 6
    assert _only_strip_reset(*_strip_case(other))
    cnt, src_cnt = _strip_case(other, match_triangle=False)
    assert np.array_equal(cnt, src_cnt)

    def none(src, aov):
        aov["triangle"][:, STRIP] = 6
        aov["triangle"] = None
    cnt, src_cnt = _strip_case(none)  # (no buffer on one side: nothing to match)
    assert np.array_equal(cnt, src_cnt)


def test_empty_source_pixel_resets():
    def empty(src, aov):
        src[2][:, STRIP] = 0
    cnt, src_cnt = _strip_case(empty)
    assert (cnt[:, STRIP] == 0).all() and np.array_equal(cnt, src_cnt)

    def missed(src, aov):
        aov["depth"][:, STRIP] = np.inf
    assert _only_strip_reset(*_strip_case(missed))


def test_point_behind_the_old_camera_resets():
    W, H = 64, 48
    src, aov_a, cam_a, aov_b, cam_b = ref.plane_case(W, H, 4.0)
    past = ref.camera((cam_a.position.x, cam_a.position.y, cam_a.position.z + 8.0), 0.0, 0.0, cam_a.FOV)
    fb, sq, cnt, st = _host(src, aov_a, past, aov_b, cam_b)
    assert (cnt == 0).all() and not fb.any() and not sq.any() and st["kept_pixels"] == 0


def test_projection_off_the_frame_resets():
    W, H = 64, 48
    for shift in (dict(shift_x=W + 5), dict(shift_x=-(W + 5)), dict(shift_y=H + 5), dict(shift_y=-(H + 5))):
        src, aov_a, cam_a, aov_b, cam_b = ref.plane_case(W, H, 4.0, **shift)
        fb, sq, cnt, st = _host(src, aov_a, cam_a, aov_b, cam_b)
        assert (cnt == 0).all() and not fb.any() and not sq.any(), shift


def test_non_finite_inputs_stay_in_bounds():
    """NaN / Inf depths and cameras: every pixel resets or keeps finite sums, and nothing is written outside
    the output arrays (canaries on both sides of each)"""
    L = rt.lib()
    W, H = 67, 45
    n = W * H
    pad = 256
    for name in ("nan_depth", "nan_camera", "inf_camera", "nan_src_camera"):
        src, aov_a, cam_a, aov_b, cam_b, _ = ref.case(name, W, H)
        arrs = [np.ascontiguousarray(a) for a in (src[0], src[1], src[2], aov_a["depth"], aov_a["normal"],
                                                  aov_a["triangle"], aov_b["depth"], aov_b["normal"],
                                                  aov_b["triangle"])]
        outs = [np.full(pad + n * per + pad, 0x5A5A5A5A, np.uint32) for per in (3, 1, 1)]
        st = np.zeros(3, np.uint64)
        p = [a.ctypes.data for a in arrs]
        rc = L.rt_reproject_host(p[0], p[1], p[2], p[3], p[4], p[5], cam_a, p[6], p[7], p[8], cam_b, W, H,
                                 *[o.ctypes.data + 4 * pad for o in outs], st.ctypes.data, None)
        assert rc == 0, name
        for o in outs:
            assert (o[:pad] == 0x5A5A5A5A).all() and (o[-pad:] == 0x5A5A5A5A).all(), name
        assert np.isfinite(outs[0][pad:-pad].view(F)).all() and np.isfinite(outs[1][pad:-pad].view(F)).all()
        cnt = outs[2][pad:-pad].view(np.int32)
        assert (cnt >= 0).all() and (cnt <= 64).all()


# ---------------------------------------------------------------- the interface
def test_header_and_binding(tmp_path):
    text = open(os.path.join(INC, "isaklm_rt.h")).read()
    assert int(re.search(r"#define RT_ABI_VERSION (\d+)", text).group(1)) == 12  # an addition within ABI 12
    assert re.search(r"^#define RT_HAS_REPROJECT 1$", text, re.M)
    fields = [name for name, _ in rt.RtReprojectOptions._fields_]
    assert fields == ["max_history", "depth_tol", "normal_min", "match_triangle", "stream", "stats_device"]
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "isaklm_rt.h"\n#ifndef RT_HAS_REPROJECT\n'
                   '#error "no feature test"\n#endif\n#if RT_HAS_REPROJECT != 1 || !defined(RT_HAS_TRACE_PATHS)\n'
                   '#error "feature tests"\n#endif\nint main(void) {\n  printf("%zu", sizeof(RtReprojectOptions));\n'
                   + "".join(f'  printf(" %zu", offsetof(RtReprojectOptions, {f}));\n' for f in fields)
                   + "  return 0;\n}\n")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", INC, str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [ctypes.sizeof(rt.RtReprojectOptions)] + [getattr(rt.RtReprojectOptions, f).offset for f in fields]
    o = rt.RtReprojectOptions(9, 9.0, 9.0, 9, 9, 9)
    rt.lib().rt_default_reproject_options(ctypes.byref(o))
    assert (o.max_history, o.match_triangle, o.stream, o.stats_device) == (64, 1, None, None)
    assert (F(o.depth_tol), F(o.normal_min)) == (F(0.02), F(0.95))
    assert rt.REPROJECT_STATS == ("pixels", "kept_pixels", "carried_samples")


def test_zero_options_are_the_defaults():
    W, H = 64, 48
    src, aov_a, cam_a, aov_b, cam_b, _ = ref.case("small_move", W, H)
    a = _host(src, aov_a, cam_a, aov_b, cam_b)
    b = _host(src, aov_a, cam_a, aov_b, cam_b, max_history=64, depth_tol=0.02, normal_min=0.95, match_triangle=True)
    _same(a, b)
    L = rt.lib()
    arrs = [np.ascontiguousarray(x) for x in (src[0], src[1], src[2], aov_a["depth"], aov_a["normal"],
                                              aov_a["triangle"], aov_b["depth"], aov_b["normal"], aov_b["triangle"])]
    p = [x.ctypes.data for x in arrs]
    outs = [np.zeros((H, W, 3), F), np.zeros((H, W), F), np.zeros((H, W), np.int32)]
    assert L.rt_reproject_host(*p[:6], cam_a, *p[6:], cam_b, W, H, *[o.ctypes.data for o in outs], None, None) == 0
    _same(outs, a)  # opt NULL, stats NULL


BAD_OPTIONS = [dict(max_history=-1), dict(max_history=(1 << 20) + 1), dict(depth_tol=-0.01),
               dict(depth_tol=float("nan")), dict(depth_tol=float("inf")), dict(depth_tol=float("-inf")),
               dict(normal_min=-1.0), dict(normal_min=1.5), dict(normal_min=float("nan")),
               dict(normal_min=float("inf")), dict(normal_min=-2.0)]


def test_host_argument_errors():
    L = rt.lib()
    W, H = 4, 3
    src, aov_a, cam_a, aov_b, cam_b, _ = ref.case("unmoved", W, H)
    arrs = [np.ascontiguousarray(x) for x in (src[0], src[1], src[2], aov_a["depth"], aov_a["normal"],
                                              aov_a["triangle"], aov_b["depth"], aov_b["normal"], aov_b["triangle"])]
    outs = [np.zeros((H, W, 3), F), np.zeros((H, W), F), np.zeros((H, W), np.int32)]
    st = np.zeros(3, np.uint64)

    def call(p, q, w=W, h=H, o=None):
        return L.rt_reproject_host(*p[:6], cam_a, *p[6:], cam_b, w, h, *q, st.ctypes.data,
                                   None if o is None else ctypes.byref(o))
    p = [x.ctypes.data for x in arrs]
    q = [x.ctypes.data for x in outs]
    assert call(p, q) == 0
    for i in range(9):
        bad = list(p)
        bad[i] = None
        assert call(bad, q) == (0 if i in (5, 8) else E_INVALID), i  # (the triangle buffers are optional)
    assert L.rt_last_error()
    for i in range(3):
        bad = list(q)
        bad[i] = None
        assert call(p, bad) == E_INVALID, i
    for w, h in ((0, 3), (4, 0), (-1, 3), (4, -2), (1 << 16, 1 << 15)):
        assert call(p, q, w, h) == E_INVALID, (w, h)
    # dst over src: the same array, a shifted view of it, and one array of the other kind
    assert call(p, [p[0], q[1], q[2]]) == E_INVALID
    assert call(p, [q[0], p[1] + 4, q[2]]) == E_INVALID
    assert call(p, [q[0], q[1], p[2] + 4 * (W * H - 1)]) == E_INVALID
    assert call(p, [q[0], p[2], q[2]]) == E_INVALID
    for bad in BAD_OPTIONS:
        assert call(p, q, o=rt.reproject_options(**bad)) == E_INVALID, bad
    o = rt.reproject_options()
    o.match_triangle = 2
    assert call(p, q, o=o) == E_INVALID
    o.match_triangle = -2
    assert call(p, q, o=o) == E_INVALID


def test_device_argument_errors_without_a_device():
    """rt_reproject rejects these before any GPU call: the pointers below are not device memory"""
    L = rt.lib()
    a, b = 0x100000, 0x900000  # two frames far apart
    gs = rt.G_Buffer(a, a + 0x10000, a + 0x20000, a + 0x30000)
    gd = rt.G_Buffer(b, b + 0x10000, b + 0x20000, a + 0x30000)  # (the shared RNG array is allowed)
    aov = rt.RtAovBuffers(0x2000, 0x3000, None, None)
    cam = ref.camera((0, 0, 0))

    def call(gs=gs, sa=aov, da=aov, w=8, h=8, gd=gd, o=None):
        return L.rt_reproject(gs, None if sa is None else ctypes.byref(sa), cam,
                              None if da is None else ctypes.byref(da), cam, w, h, gd,
                              None if o is None else ctypes.byref(o))
    for i in range(3):
        f = [a, a + 0x10000, a + 0x20000, a + 0x30000]
        f[i] = None
        assert call(gs=rt.G_Buffer(*f)) == E_INVALID
        f = [b, b + 0x10000, b + 0x20000, None]
        f[i] = None
        assert call(gd=rt.G_Buffer(*f)) == E_INVALID
    assert L.rt_last_error()
    assert call(sa=None) == E_INVALID and call(da=None) == E_INVALID
    assert call(sa=rt.RtAovBuffers(None, 0x3000, None, None)) == E_INVALID
    assert call(da=rt.RtAovBuffers(0x2000, None, None, None)) == E_INVALID
    for w, h in ((0, 8), (8, 0), (-1, 8), (1 << 16, 1 << 15)):
        assert call(w=w, h=h) == E_INVALID, (w, h)
    assert call(gd=rt.G_Buffer(a, b + 0x10000, b + 0x20000, None)) == E_INVALID  # dst fb = src fb
    assert call(gd=rt.G_Buffer(b, a + 0x10000 + 64, b + 0x20000, None)) == E_INVALID  # dst sq inside src sq
    assert call(gd=rt.G_Buffer(b, b + 0x10000, a + 8 * 8 * 12 - 4, None)) == E_INVALID  # dst count on src fb's end
    for bad in BAD_OPTIONS:
        assert call(o=rt.reproject_options(**bad)) == E_INVALID, bad
