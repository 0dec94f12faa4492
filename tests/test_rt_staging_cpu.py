"""The numpy-level wrappers of rt.py without a GPU: what they stage, in which order, and what they hand back.

A shim stands in for the library (installed as rt._lib, the real one restored after each test).  It treats host
memory as device memory: rt_device_alloc / rt_free / rt_upload / rt_download / rt_memset act on host buffers, a
G_Buffer is four host arrays, and it counts what is allocated.  The device calls that have a host twin
(rt_sampler_rays, rt_convergence, rt_denoise[_sampler], rt_reproject[_sampler]) are forwarded to it, so the
wrappers must equal the *_host wrappers bit for bit.  Every other device call checks the staging itself: the shim
keeps the bytes it finds behind the input pointers and writes a fill byte of its own into every output and a
known word into every stats slot."""
import ctypes
import types

import numpy as np
import pytest

import denoise_ref as dref
import model_frames_ref as mf
import reproject_ref as rref
import rt

F = np.float32
U64 = ctypes.c_ulonglong
SCENE = types.SimpleNamespace(prepared=ctypes.c_void_p(0x5CE0))
STATS_WORD = 0x5100  # stats slot i leaves a call as STATS_WORD + i
FRESH = 0xEE  # every byte of a new allocation


def _a(p):
    """the address in whatever stands for a void * argument"""
    p = getattr(p, "_as_parameter_", p)
    if isinstance(p, ctypes.c_void_p):
        p = p.value
    return int(p or 0)


class Shim:
    def __init__(self, real):
        self.real = real
        self.live = {}   # address -> (size, the numpy array that holds it)
        self.calls = []  # names, in order
        self.seen = {}   # what the last checked call found behind its pointers
        self.fail = None  # the name of a call that is to return an error
        self.allocs = 0

    def __getattr__(self, name):
        return getattr(self.real, name)

    # ---- memory
    def _new(self, nbytes):
        hold = np.full(nbytes + 128, FRESH, np.uint8)
        addr = (hold.ctypes.data + 63) & ~63
        self.live[addr] = (nbytes, hold)
        return addr

    def _inside(self, addr, n):
        assert any(b <= addr and addr + n <= b + size for b, (size, _) in self.live.items()), \
            f"{n} bytes at {addr:#x} are not inside a live allocation"

    def take(self, p, n):
        self._inside(_a(p), n)
        return ctypes.string_at(_a(p), n)

    def fill(self, p, n, byte):
        self._inside(_a(p), n)
        ctypes.memset(_a(p), byte, n)

    def stats(self, p, words):
        """the words found in a stats block (None: no block), which then holds STATS_WORD + i"""
        if not _a(p):
            return None
        self._inside(_a(p), 8 * words)
        a = (U64 * words).from_address(_a(p))
        found = list(a)
        a[:] = [STATS_WORD + i for i in range(words)]
        return found

    def _rc(self, name):
        self.calls.append(name)
        return -1 if self.fail == name else 0

    def rt_device_alloc(self, out, nbytes):
        assert nbytes >= 16
        self.allocs += 1
        out._obj.value = self._new(nbytes)
        return self._rc("rt_device_alloc")

    def rt_free(self, p):
        del self.live[_a(p)]
        return self._rc("rt_free")

    def rt_upload(self, dst, src, n):
        assert n > 0
        self._inside(_a(dst), n)
        ctypes.memmove(_a(dst), _a(src), n)
        return self._rc("rt_upload")

    def rt_download(self, dst, src, n):
        assert n > 0
        self._inside(_a(src), n)
        ctypes.memmove(_a(dst), _a(src), n)
        return self._rc("rt_download")

    def rt_memset(self, p, value, n):
        self.fill(p, n, value)
        return self._rc("rt_memset")

    def rt_synchronize(self):
        return self._rc("rt_synchronize")

    def rt_join(self, stream):
        return self._rc("rt_join")

    def rt_gbuffer_create(self, width, height, seed_skip, out):
        n = width * height
        g = out._obj
        g.frame_buffer, g.squared_luminance, g.sample_count, g.random_numbers = (self._new(max(k * n, 16))
                                                                                 for k in (12, 4, 4, 4))
        for p, k in ((g.frame_buffer, 12), (g.squared_luminance, 4), (g.sample_count, 4)):
            ctypes.memset(p, 0, k * n)
        assert self.real.rt_gbuffer_seeds(g.random_numbers, n, seed_skip) == 0
        return self._rc("rt_gbuffer_create")

    def rt_gbuffer_destroy(self, ref):
        g = ref._obj
        for name, _ in rt.G_Buffer._fields_:
            del self.live[getattr(g, name)]
            setattr(g, name, None)
        return self._rc("rt_gbuffer_destroy")

    # ---- the calls with a host twin
    def rt_sampler_rays(self, smp, rng, n, rays, stream):
        s = smp._obj
        self.seen = dict(pixels=s.pixels_device, points=s.points_device, rng=_a(rng))
        return self._rc("rt_sampler_rays") or self.real.rt_sampler_rays_host(smp, _a(rng) or None, n, _a(rays))

    def rt_convergence(self, rad, sq, cnt, n, min_samples, tolerance, err, stats, stream):
        st = (U64 * 4)()
        self.seen = dict(err=_a(err))
        rc = self._rc("rt_convergence") or self.real.rt_convergence_host(_a(rad), _a(sq), _a(cnt), n, min_samples,
                                                                         tolerance, _a(err) or None, st)
        self._add(stats, st)
        return rc

    def _add(self, stats, st):  # (the device calls add to the block, their twins write it)
        if _a(stats):
            self._inside(_a(stats), 8 * len(st))
            block = (U64 * len(st)).from_address(_a(stats))
            block[:] = [a + b for a, b in zip(block, st)]

    def rt_denoise(self, g, aov, width, height, out, opt):
        b = aov._obj
        assert not b.triangle
        return self._rc("rt_denoise") or self.real.rt_denoise_host(
            g.frame_buffer, g.squared_luminance, g.sample_count, b.depth, b.normal, b.albedo, width, height, _a(out), opt)

    def rt_denoise_sampler(self, g, aov, smp, out, opt):
        b = aov._obj
        self.seen = dict(pixels=smp._obj.pixels_device)
        return self._rc("rt_denoise_sampler") or self.real.rt_denoise_sampler_host(
            g.frame_buffer, g.squared_luminance, g.sample_count, b.depth, b.normal, b.albedo, smp, _a(out), opt)

    def rt_reproject(self, gs, bs, cam_s, bd, cam_d, width, height, gd, opt):
        bs, bd, st = bs._obj, bd._obj, (U64 * 3)()
        self.seen = dict(stats=opt._obj.stats_device)
        rc = self._rc("rt_reproject") or self.real.rt_reproject_host(
            gs.frame_buffer, gs.squared_luminance, gs.sample_count, bs.depth, bs.normal, bs.triangle, cam_s, bd.depth,
            bd.normal, bd.triangle, cam_d, width, height, gd.frame_buffer, gd.squared_luminance, gd.sample_count, st, opt)
        self._add(opt._obj.stats_device, st)
        return rc

    def rt_reproject_sampler(self, gs, bs, smp_s, bd, smp_d, gd, opt):
        bs, bd, st = bs._obj, bd._obj, (U64 * 3)()
        self.seen = dict(stats=opt._obj.stats_device)
        rc = self._rc("rt_reproject_sampler") or self.real.rt_reproject_sampler_host(
            gs.frame_buffer, gs.squared_luminance, gs.sample_count, bs.depth, bs.normal, bs.triangle, smp_s, bd.depth,
            bd.normal, bd.triangle, smp_d, gd.frame_buffer, gd.squared_luminance, gd.sample_count, st, opt)
        self._add(opt._obj.stats_device, st)
        return rc

    # ---- the calls without one: keep the inputs, fill the outputs
    def rt_trace_rays(self, scene, rays, n, hits, surf, opt):
        o = opt._obj
        self.seen = dict(scene=_a(scene), rays=self.take(rays, 24 * n), n=n, surface=bool(_a(surf)),
                         stats=self.stats(o.stats_device, 3), traversal=o.traversal, stream=o.stream)
        self.fill(hits, 16 * n, 0xA1)
        if _a(surf):
            self.fill(surf, 80 * n, 0xA2)
        return self._rc("rt_trace_rays")

    def rt_occluded(self, scene, rays, tmax, n, out, opt):
        o = opt._obj
        self.seen = dict(scene=_a(scene), rays=self.take(rays, 24 * n), n=n, stats=self.stats(o.stats_device, 3),
                         tmax=self.take(tmax, 4 * n) if _a(tmax) else None, traversal=o.traversal, stream=o.stream)
        self.fill(out, n, 0xA3)
        return self._rc("rt_occluded")

    def _paths(self, name, rng, n, rad, sq, cnt, opt, **more):
        o = opt._obj
        self.seen = dict(n=n, rng=self.take(rng, 4 * n), radiance=self.take(rad, 12 * n), sq=self.take(sq, 4 * n),
                         count=self.take(cnt, 4 * n) if _a(cnt) else None, stats=self.stats(o.stats_device, 5),
                         samples=o.samples, max_depth=o.max_depth, accumulate=o.accumulate, traversal=o.traversal,
                         stream=o.stream, **more)
        for p, k, byte in ((rad, 12, 0xB1), (sq, 4, 0xB2), (rng, 4, 0xB3), (cnt, 4, 0xB4)):
            if _a(p):
                self.fill(p, k * n, byte)
        return self._rc(name)

    def rt_trace_paths(self, scene, rays, rng, n, rad, sq, opt):
        return self._paths("rt_trace_paths", rng, n, rad, sq, None, opt, rays=self.take(rays, 24 * n))

    def _sampler(self, smp, n):
        s = smp._obj
        pix, pts = s.pixels_device, s.points_device
        return dict(kind=s.kind, size=(s.width, s.height), pixels=pix, points=pts,
                    pixel_list=self.take(pix, 4 * n) if pix not in (None, 4) else None,
                    point_list=self.take(pts, 24 * n) if pts not in (None, 8) else None)

    def rt_sample_paths(self, scene, smp, rng, n, rad, sq, cnt, opt):
        return self._paths("rt_sample_paths", rng, n, rad, sq, cnt, opt, sampler=self._sampler(smp, n), adaptive=None)

    def rt_sample_paths_adaptive(self, scene, smp, rng, n, rad, sq, cnt, opt, ad):
        return self._paths("rt_sample_paths_adaptive", rng, n, rad, sq, cnt, opt, sampler=self._sampler(smp, n),
                           adaptive=(ad._obj.min_samples, ad._obj.tolerance))

    def _aov(self, b, n):
        for p, k, byte in ((b.depth, 4, 0xC1), (b.normal, 12, 0xC2), (b.albedo, 12, 0xC3), (b.triangle, 4, 0xC4)):
            self.fill(p, k * n, byte)

    def rt_render_aov(self, scene, camera, width, height, aov, opt):
        self.seen = dict(scene=_a(scene), camera=camera.as_list(), size=(width, height), traversal=opt._obj.traversal)
        self._aov(aov._obj, width * height)
        return self._rc("rt_render_aov")

    def rt_sample_aov(self, scene, smp, n, aov, opt):
        o = opt._obj
        self.seen = dict(scene=_a(scene), n=n, sampler=self._sampler(smp, n), stats=self.stats(o.stats_device, 3),
                         traversal=o.traversal)
        self._aov(aov._obj, n)
        return self._rc("rt_sample_aov")

    def rt_camera_rays(self, camera, width, height, rays, stream):
        self.seen = dict(camera=camera.as_list(), size=(width, height))
        self.fill(rays, 24 * width * height, 0xD1)
        return self._rc("rt_camera_rays")

    def rt_tonemap_rgb(self, rgb, out, width, height, stream):
        self.seen = dict(rgb=self.take(rgb, 12 * width * height), size=(width, height))
        self.fill(out, 4 * width * height, 0xD2)
        return self._rc("rt_tonemap_rgb")

    def rt_tonemap(self, g, out, width, height, stream):
        self.seen = dict(fb=g.frame_buffer, size=(width, height))
        self.fill(out, 4 * width * height, 0xD3)
        return self._rc("rt_tonemap")


@pytest.fixture
def shim():
    real = rt.lib()
    s = Shim(real)
    rt._lib = s
    try:
        yield s
    finally:
        rt._lib = real
    assert not s.live, "a device allocation outlived its call"


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def is_fill(a, byte, shape, dtype):
    return a.shape == shape and a.dtype == dtype and a.flags["C_CONTIGUOUS"] and \
        (np.frombuffer(a.tobytes(), np.uint8) == byte).all()


def transfers(shim):
    return [c for c in shim.calls if c in ("rt_upload", "rt_download")]


def raises_unallocated(shim, fn, *args, **kw):
    before, live = shim.allocs, set(shim.live)
    with pytest.raises(ValueError):
        fn(*args, **kw)
    assert shim.allocs == before and set(shim.live) == live


def fails_clean(shim, name, fn, *args, **kw):
    """the C call returns an error: RtError, and nothing stays allocated"""
    live = set(shim.live)
    shim.fail = name
    try:
        with pytest.raises(rt.RtError):
            fn(*args, **kw)
    finally:
        shim.fail = None
    assert set(shim.live) == live


def rays_of(n, seed=3):
    return np.random.default_rng(seed).normal(size=(n, 6)).astype(F)


QUERY_WORDS = {k: STATS_WORD + i for i, k in enumerate(rt.QUERY_STATS)}
PATH_WORDS = {k: STATS_WORD + i for i, k in enumerate(rt.PATH_STATS)}


# ---------------------------------------------------------------- the forwarded calls: bit for bit the host twins
def _samplers():
    W, H = 7, 5
    out = {kind: mf.sampler(kind, W, H, **mf.CAM_ROTATED) for kind in mf.KINDS}
    pts = rays_of(11, 8)
    out["hemisphere"] = rt.Sampler("hemisphere", points=pts)
    out["pixel list"] = mf.sampler("fisheye", W, H, **mf.CAM_ROTATED, pixels=[0, 3, 34, 35, -1, 17])
    return out


@pytest.mark.parametrize("name", ["pinhole", "equirect", "fisheye", "ortho", "hemisphere", "pixel list"])
def test_sampler_rays_equals_host(shim, name):
    smp = _samplers()[name]
    rng = rt.seeds(smp.n, 5)
    keep = rng.copy()
    rays, out = rt.sampler_rays(smp, rng)
    want_rays, want_out = rt.sampler_rays_host(smp, rng)
    assert rays.shape == (smp.n, 6) and same_bits(rays, want_rays) and same_bits(out, want_out)
    assert out is not rng and np.array_equal(rng, keep) and not np.array_equal(out, keep)
    if name != "hemisphere":
        centre = rt.sampler_rays(smp)
        assert isinstance(centre, np.ndarray) and same_bits(centre, rt.sampler_rays_host(smp))
        assert shim.seen["rng"] == 0
    raises_unallocated(shim, rt.sampler_rays, smp, rng[:-1])
    raises_unallocated(shim, rt.sampler_rays, smp, rng.astype(np.int32))
    fails_clean(shim, "rt_sampler_rays", rt.sampler_rays, smp, rng)


def test_sampler_rays_of_empty_lists(shim):
    """an empty list still is a list: the library sees the dummy pointers 4 and 8, and nothing is copied"""
    smp = mf.sampler("pinhole", 7, 5, pixels=np.zeros(0, np.int32))
    rays, out = rt.sampler_rays(smp, np.zeros(0, np.uint32))
    assert rays.shape == (0, 6) and rays.dtype == F and out.shape == (0,) and out.dtype == np.uint32
    assert shim.seen["pixels"] == 4 and shim.seen["points"] is None and not transfers(shim)
    assert same_bits(rays, rt.sampler_rays_host(smp, np.zeros(0, np.uint32))[0])
    assert rt.sampler_rays(smp).shape == (0, 6)
    smp = rt.Sampler("hemisphere", points=np.zeros((0, 6), F))
    rays, out = rt.sampler_rays(smp, np.zeros(0, np.uint32))
    assert rays.shape == (0, 6) and shim.seen["points"] == 8 and shim.seen["pixels"] is None and not transfers(shim)


def test_convergence_equals_host(shim):
    fb, sq, count = rref.sums(9, 7, 7)
    keep = [a.copy() for a in (fb, sq, count)]
    for tol in (0.05, 0.5):
        assert rt.convergence(fb, sq, count, 2, tol) == rt.convergence_host(fb, sq, count, 2, tol)
        assert shim.seen["err"] == 0
        st, err = rt.convergence(fb, sq, count, 2, tol, rel_error=True)
        want_st, want_err = rt.convergence_host(fb, sq, count, 2, tol, rel_error=True)
        assert st == want_st and st["elements"] == 63 and err.shape == (63,) and same_bits(err, want_err)
    assert all(np.array_equal(a, b) for a, b in zip((fb, sq, count), keep))
    empty = (np.zeros((0, 3), F), np.zeros(0, F), np.zeros(0, np.int32))
    assert rt.convergence(*empty, 2, 0.05) == rt.convergence_host(*empty, 2, 0.05)
    st, err = rt.convergence(*empty, 2, 0.05, rel_error=True)
    assert st == dict.fromkeys(rt.CONVERGENCE_STATS, 0) and err.shape == (0,) and err.dtype == F
    assert shim.seen["err"] == 0
    raises_unallocated(shim, rt.convergence, fb, sq[:-1], count, 2, 0.05)
    fails_clean(shim, "rt_convergence", rt.convergence, fb, sq, count, 2, 0.05)


def _gbuffer(sums, W, H, seed_skip=0):
    g = rt.GBuffer(W, H, seed_skip)
    g.upload(sums[0], sums[1], sums[2], g.download()[3])
    return g


@pytest.mark.parametrize("shape", [(9, 7), (1, 5)], ids=["9x7", "1x5"])
def test_denoise_equals_host(shim, shape):
    W, H = shape
    f = dref.synthetic_frame(W, H)
    sums = (f["fb"], f["sq"], f["count"])
    host = lambda smp=None, **o: (rt.denoise_host(*sums, f["depth"], f["normal"], f["albedo"], **o) if smp is None else  # noqa: E731
                                  rt.denoise_sampler_host(*sums, f["depth"], f["normal"], f["albedo"], smp, **o))
    held = {k: np.ascontiguousarray(f[k], F) for k in ("depth", "normal", "albedo")}
    pointers = {k: a.ctypes.data for k, a in held.items()}
    eq, fish = mf.sampler("equirect", W, H), mf.sampler("fisheye", W, H)
    g = _gbuffer(sums, W, H)
    try:
        for aov in (f, pointers, {k: ctypes.c_void_p(p) for k, p in pointers.items()}):
            live = len(shim.live)
            plain = rt.denoise(g, aov)
            assert plain.shape == (H, W, 3) and plain.dtype == F and same_bits(plain, host())
            assert same_bits(rt.denoise(g, aov, iterations=2, sigma_lum=2.0), host(iterations=2, sigma_lum=2.0))
            wrapped = rt.denoise_sampler(g, aov, eq)
            assert same_bits(wrapped, host(eq)) and shim.seen["pixels"] is None
            assert same_bits(rt.denoise_sampler(g, aov, fish), host(fish)) and same_bits(host(fish), plain)
            if W > 1:  # the seam: an equirect frame's first column has neighbours in its last
                assert not same_bits(wrapped[:, 0], plain[:, 0])
            assert len(shim.live) == live
        no_albedo = {k: f[k] for k in ("depth", "normal")}
        assert same_bits(rt.denoise(g, no_albedo, demodulate=False),
                         rt.denoise_host(*sums, f["depth"], f["normal"], None, demodulate=False))
        assert "rt_synchronize" not in shim.calls
        rt.denoise(g, f, stream=0x77)
        assert shim.calls.count("rt_synchronize") == 1
        raises_unallocated(shim, rt.denoise_sampler, g, f, mf.sampler("equirect", W + 1, H))
        live = len(shim.live)
        with pytest.raises(ValueError):
            rt.denoise(g, dict(f, normal=f["normal"][:, :, :2]))
        assert len(shim.live) == live
        fails_clean(shim, "rt_denoise", rt.denoise, g, f)
        fails_clean(shim, "rt_denoise_sampler", rt.denoise_sampler, g, f, eq)
    finally:
        g.free()


def _reproject_cases():
    src, aov_a, cam_a, aov_b, cam_b, _ = rref.case("small_move", 9, 7)
    yield "cameras", rt.reproject, rt.reproject_host, src, aov_a, cam_a, aov_b, cam_b
    src, aov_a, smp_a, aov_b, smp_b = mf.moved_case("equirect", 9, 7)
    yield "samplers", rt.reproject_sampler, rt.reproject_sampler_host, src, aov_a, smp_a, aov_b, smp_b


@pytest.mark.parametrize("case", _reproject_cases(), ids=lambda c: c[0])
def test_reproject_equals_host(shim, case):
    _, device, host, src, aov_a, cam_a, aov_b, cam_b = case
    W, H = 9, 7
    names = ("depth", "normal", "triangle")
    held = [{k: np.ascontiguousarray(aov[k]) for k in names} for aov in (aov_a, aov_b)]
    pointers = [{k: a.ctypes.data for k, a in side.items()} for side in held]
    g = _gbuffer(src, W, H, seed_skip=40)
    given = rt.GBuffer(W, H, seed_skip=900)
    try:
        for opts in ({}, dict(max_history=16, depth_tol=0.05, match_triangle=False)):
            *want, want_st = host(*src, aov_a, cam_a, aov_b, cam_b, stats=True, **opts)
            assert want_st["pixels"] == W * H and want_st["kept_pixels"] > 0
            for a, b in ((aov_a, aov_b), pointers):
                live = len(shim.live)
                out, st = device(g, a, cam_a, b, cam_b, stats=True, **opts)
                try:
                    fb, sq, cnt, rng = out.download()
                finally:
                    out.free()
                assert st == want_st and all(same_bits(x, y.reshape(x.shape)) for x, y in zip((fb, sq, cnt), want))
                assert np.array_equal(rng, rt.seeds(W * H, 40))  # a new G-buffer carries the source's RNG states on
                assert len(shim.live) == live
            assert device(g, aov_a, cam_a, aov_b, cam_b, out=given, stats=True, **opts) == (given, want_st)
            assert device(g, aov_a, cam_a, aov_b, cam_b, out=given, **opts) is given and shim.seen["stats"] is None
            fb, sq, cnt, rng = given.download()
            assert all(same_bits(x, y.reshape(x.shape)) for x, y in zip((fb, sq, cnt), want))
            assert np.array_equal(rng, rt.seeds(W * H, 900))  # `out`'s own are left alone
        assert "rt_synchronize" not in shim.calls
        device(g, aov_a, cam_a, aov_b, cam_b, out=given, stream=0x77)
        assert shim.calls.count("rt_synchronize") == 1
        small = rt.GBuffer(W - 1, H)
        try:
            raises_unallocated(shim, device, g, aov_a, cam_a, aov_b, cam_b, out=small)
        finally:
            small.free()
        live = len(shim.live)
        with pytest.raises(ValueError):
            device(g, dict(aov_a, depth=aov_a["depth"][1:]), cam_a, aov_b, cam_b, out=given)
        assert len(shim.live) == live
        fails_clean(shim, device.__name__.replace("reproject", "rt_reproject"), device, g, aov_a, cam_a, aov_b, cam_b,
                    out=given, stats=True)
    finally:
        g.free()
        given.free()


# ---------------------------------------------------------------- the other calls: the staging itself
@pytest.mark.parametrize("surface", [False, True])
@pytest.mark.parametrize("stats", [False, True])
def test_trace_rays_staging(shim, surface, stats):
    rays = rays_of(13)
    keep = rays.copy()
    out = rt.trace_rays(SCENE, rays, surface=surface, traversal=rt.TRAVERSAL_KD, stats=stats)
    out = out if isinstance(out, tuple) else (out,)
    assert len(out) == 1 + surface + stats
    assert is_fill(out[0], 0xA1, (13,), rt.RAY_HIT)
    assert not surface or is_fill(out[1], 0xA2, (13,), rt.RAY_SURFACE)
    assert not stats or out[-1] == QUERY_WORDS
    seen = shim.seen
    assert seen["scene"] == 0x5CE0 and seen["rays"] == keep.tobytes() and seen["n"] == 13
    assert seen["surface"] is surface and seen["stats"] == ([0, 0, 0] if stats else None)
    assert seen["traversal"] == rt.TRAVERSAL_KD and seen["stream"] is None
    assert np.array_equal(rays, keep) and "rt_synchronize" not in shim.calls
    assert ("rt_memset" in shim.calls) is stats
    assert same_bits(rt.trace_rays(SCENE, rays.astype(np.float64).tolist(), stream=0x77), out[0])  # (any array-like)
    assert shim.seen["stream"] == 0x77 and shim.seen["rays"] == keep.tobytes()
    assert shim.calls.count("rt_synchronize") == 1
    fails_clean(shim, "rt_trace_rays", rt.trace_rays, SCENE, rays, surface=surface, stats=stats)
    fails_clean(shim, "rt_download", rt.trace_rays, SCENE, rays, surface=surface, stats=stats)


def test_trace_rays_of_nothing_and_of_the_wrong_shape(shim):
    hits, surf = rt.trace_rays(SCENE, np.zeros((0, 6), F), surface=True)
    assert hits.shape == (0,) and hits.dtype == rt.RAY_HIT and surf.shape == (0,) and surf.dtype == rt.RAY_SURFACE
    assert shim.seen["n"] == 0 and not transfers(shim)
    raises_unallocated(shim, rt.trace_rays, SCENE, np.zeros((4, 5), F))
    raises_unallocated(shim, rt.trace_rays, SCENE, np.zeros(6, F))


@pytest.mark.parametrize("stats", [False, True])
def test_occluded_staging(shim, stats):
    rays = rays_of(13)
    keep = rays.copy()
    for tmax, want in ((None, None), (2.5, np.full(13, 2.5, F)), (np.arange(13.0), np.arange(13, dtype=F))):
        out = rt.occluded(SCENE, rays, tmax, stats=stats)
        if stats:
            assert isinstance(out, tuple) and len(out) == 2 and out[1] == {k: STATS_WORD + i for i, k in
                                                                           enumerate(rt.OCCLUSION_STATS)}
            out = out[0]
        assert is_fill(out, 0xA3, (13,), np.uint8)
        seen = shim.seen
        assert seen["rays"] == keep.tobytes() and seen["tmax"] == (None if want is None else want.tobytes())
        assert seen["stats"] == ([0, 0, 0] if stats else None) and seen["stream"] is None
    assert np.array_equal(rays, keep) and "rt_synchronize" not in shim.calls
    rt.occluded(SCENE, rays, stream=0x77)
    assert shim.calls.count("rt_synchronize") == 1 and shim.seen["stream"] == 0x77
    shim.calls.clear()
    out = rt.occluded(SCENE, np.zeros((0, 6), F), np.zeros(0, F))
    assert out.shape == (0,) and out.dtype == np.uint8 and not transfers(shim)
    raises_unallocated(shim, rt.occluded, SCENE, np.zeros((4, 5), F))
    raises_unallocated(shim, rt.occluded, SCENE, rays, np.zeros(12, F))
    raises_unallocated(shim, rt.occluded, SCENE, rays, np.zeros((13, 1), F))
    fails_clean(shim, "rt_occluded", rt.occluded, SCENE, rays, 1.0, stats=stats)


def _path_outputs(out, n, count, stats):
    assert isinstance(out, tuple) and len(out) == 3 + count + stats
    assert is_fill(out[0], 0xB1, (n, 3), F) and is_fill(out[1], 0xB2, (n,), F) and is_fill(out[2], 0xB3, (n,), np.uint32)
    assert not count or is_fill(out[3], 0xB4, (n,), np.int32)
    assert not stats or out[-1] == PATH_WORDS


@pytest.mark.parametrize("stats", [False, True])
def test_trace_paths_staging(shim, stats):
    n = 13
    rays, rng = rays_of(n), rt.seeds(n, 9)
    rad, sq = rays_of(n)[:, :3].copy(), rays_of(n, 4)[:, 0].copy()
    keep = [a.copy() for a in (rays, rng, rad, sq)]
    for radiance, sqv in ((None, None), (rad, None), (rad, sq)):
        out = rt.trace_paths(SCENE, rays, rng, samples=3, max_depth=5, traversal=rt.TRAVERSAL_KD, stats=stats,
                             radiance=radiance, sq=sqv)
        _path_outputs(out, n, False, stats)
        seen = shim.seen
        assert seen["rays"] == rays.tobytes() and seen["rng"] == rng.tobytes() and seen["count"] is None
        assert (seen["samples"], seen["max_depth"], seen["traversal"]) == (3, 5, rt.TRAVERSAL_KD)
        assert seen["accumulate"] == (radiance is not None) and seen["stats"] == ([0] * 5 if stats else None)
        if radiance is not None:
            assert seen["radiance"] == rad.tobytes() and seen["sq"] == (sq if sqv is not None else np.zeros(n, F)).tobytes()
        assert all(o is not a for o in out[:3] for a in (rng, rad, sq))
    assert all(np.array_equal(a, b) for a, b in zip((rays, rng, rad, sq), keep))
    assert "rt_synchronize" not in shim.calls
    rt.trace_paths(SCENE, rays, rng, stream=0x77)
    assert shim.calls.count("rt_synchronize") == 1 and shim.seen["stream"] == 0x77
    shim.calls.clear()
    out = rt.trace_paths(SCENE, np.zeros((0, 6), F), np.zeros(0, np.uint32))
    assert [a.shape for a in out] == [(0, 3), (0,), (0,)] and not transfers(shim)
    raises_unallocated(shim, rt.trace_paths, SCENE, rays[:, :5], rng)
    raises_unallocated(shim, rt.trace_paths, SCENE, rays, rng.astype(np.int64))
    raises_unallocated(shim, rt.trace_paths, SCENE, rays, rng, sq=sq)
    raises_unallocated(shim, rt.trace_paths, SCENE, rays, rng, radiance=rad.astype(np.float64))
    fails_clean(shim, "rt_trace_paths", rt.trace_paths, SCENE, rays, rng, stats=stats)


@pytest.mark.parametrize("adaptive", [None, (4, 0.25)], ids=["fixed", "adaptive"])
@pytest.mark.parametrize("stats", [False, True])
def test_sample_paths_staging(shim, stats, adaptive):
    pix = np.asarray([0, 3, 34, 35, -1, 17], np.int32)
    smp = mf.sampler("fisheye", 7, 5, pixels=pix)
    n = 6
    rng = rt.seeds(n, 9)
    rad, sq, cnt = rays_of(n)[:, :3].copy(), rays_of(n, 4)[:, 0].copy(), np.arange(n, dtype=np.int32)
    keep = [a.copy() for a in (rng, rad, sq, cnt)]
    call = "rt_sample_paths" if adaptive is None else "rt_sample_paths_adaptive"
    for radiance, sqv, count in ((None, None, None), (None, None, True), (rad, sq, None), (rad, sq, True), (rad, sq, cnt)):
        if adaptive is not None and radiance is not None and count is not cnt:
            raises_unallocated(shim, rt.sample_paths, SCENE, smp, rng, radiance=radiance, sq=sqv, count=count,
                               adaptive=adaptive)
            continue
        shim.calls.clear()
        out = rt.sample_paths(SCENE, smp, rng, samples=3, max_depth=5, stats=stats, radiance=radiance, sq=sqv,
                              count=count, adaptive=adaptive)
        want_count = count is not None or adaptive is not None
        _path_outputs(out, n, want_count, stats)
        seen = shim.seen
        assert call in shim.calls and seen["adaptive"] == (None if adaptive is None else (4, 0.25))
        assert seen["rng"] == rng.tobytes() and (seen["count"] is not None) == want_count
        assert seen["accumulate"] == (radiance is not None) and seen["stats"] == ([0] * 5 if stats else None)
        assert seen["sampler"]["kind"] == rt.SAMPLER_FISHEYE and seen["sampler"]["size"] == (7, 5)
        assert seen["sampler"]["pixel_list"] == pix.tobytes() and seen["sampler"]["points"] is None
        if radiance is not None:
            assert seen["radiance"] == rad.tobytes() and seen["sq"] == sq.tobytes()
            if count is not None:  # the earlier call's counts, or zeros where only count=True is given
                assert seen["count"] == (cnt if count is cnt else np.zeros(n, np.int32)).tobytes()
    assert all(np.array_equal(a, b) for a, b in zip((rng, rad, sq, cnt), keep))
    pts = rays_of(4, 6)
    rt.sample_paths(SCENE, rt.Sampler("hemisphere", points=pts), rt.seeds(4), adaptive=adaptive)
    assert shim.seen["sampler"]["point_list"] == pts.tobytes() and shim.seen["sampler"]["pixels"] is None
    shim.calls.clear()
    out = rt.sample_paths(SCENE, mf.sampler("pinhole", 7, 5, pixels=[]), np.zeros(0, np.uint32), count=True,
                          adaptive=adaptive)
    assert [a.shape for a in out] == [(0, 3), (0,), (0,), (0,)] and shim.seen["sampler"]["pixels"] == 4
    assert not transfers(shim)
    rt.sample_paths(SCENE, rt.Sampler("hemisphere", points=np.zeros((0, 6), F)), np.zeros(0, np.uint32), adaptive=adaptive)
    assert shim.seen["sampler"]["points"] == 8 and shim.seen["sampler"]["pixels"] is None
    raises_unallocated(shim, rt.sample_paths, SCENE, smp, rng[:-1], adaptive=adaptive)
    raises_unallocated(shim, rt.sample_paths, SCENE, smp, rng, sq=sq, adaptive=adaptive)
    raises_unallocated(shim, rt.sample_paths, SCENE, smp, rng, count=cnt, adaptive=adaptive)
    raises_unallocated(shim, rt.sample_paths, SCENE, smp, rng, radiance=rad, sq=sq, count=cnt.astype(np.int64),
                       adaptive=adaptive)
    fails_clean(shim, call, rt.sample_paths, SCENE, smp, rng, stats=stats, adaptive=adaptive)


def _aov_outputs(out, lead):
    assert list(out) == ["depth", "normal", "albedo", "triangle"]
    assert is_fill(out["depth"], 0xC1, lead, F) and is_fill(out["normal"], 0xC2, lead + (3,), F)
    assert is_fill(out["albedo"], 0xC3, lead + (3,), F) and is_fill(out["triangle"], 0xC4, lead, np.int32)


def test_camera_rays_and_render_aov_staging(shim):
    cam = rref.camera((0.25, -0.5, 1.0), 0.3, 0.1)
    assert is_fill(rt.camera_rays(cam, 7, 5), 0xD1, (35, 6), F)
    assert shim.seen == dict(camera=cam.as_list(), size=(7, 5))
    fails_clean(shim, "rt_camera_rays", rt.camera_rays, cam, 7, 5)
    _aov_outputs(rt.render_aov(SCENE, cam, 7, 5, traversal=rt.TRAVERSAL_KD), (5, 7))
    assert shim.seen == dict(scene=0x5CE0, camera=cam.as_list(), size=(7, 5), traversal=rt.TRAVERSAL_KD)
    fails_clean(shim, "rt_render_aov", rt.render_aov, SCENE, cam, 7, 5)


@pytest.mark.parametrize("stats", [False, True])
def test_sample_aov_staging(shim, stats):
    pix = np.asarray([0, 3, 34, 35, -1, 17], np.int32)
    for smp, lead in ((mf.sampler("equirect", 7, 5), (5, 7)), (mf.sampler("equirect", 7, 5, pixels=pix), (6,))):
        out = rt.sample_aov(SCENE, smp, traversal=rt.TRAVERSAL_KD, stats=stats)
        if stats:
            assert isinstance(out, tuple) and len(out) == 2 and out[1] == QUERY_WORDS
            out = out[0]
        _aov_outputs(out, lead)
        seen = shim.seen
        assert seen["n"] == smp.n and seen["stats"] == ([0, 0, 0] if stats else None)
        assert seen["traversal"] == rt.TRAVERSAL_KD and seen["sampler"]["kind"] == rt.SAMPLER_EQUIRECT
        assert seen["sampler"]["pixel_list"] == (None if smp.pixels is None else pix.tobytes())
        assert seen["sampler"]["points"] is None
        fails_clean(shim, "rt_sample_aov", rt.sample_aov, SCENE, smp, stats=stats)
    shim.calls.clear()
    out = rt.sample_aov(SCENE, mf.sampler("equirect", 7, 5, pixels=[]))
    assert out["normal"].shape == (0, 3) and shim.seen["sampler"]["pixels"] == 4 and not transfers(shim)


def test_tonemap_staging(shim):
    rgb = rays_of(35)[:, :3].copy().reshape(5, 7, 3)
    keep = rgb.copy()
    assert is_fill(rt.tonemap_rgb(rgb), 0xD2, (35, 4), np.uint8)
    assert shim.seen == dict(rgb=keep.tobytes(), size=(7, 5)) and np.array_equal(rgb, keep)
    fails_clean(shim, "rt_tonemap_rgb", rt.tonemap_rgb, rgb)
    g = rt.GBuffer(7, 5)
    try:
        assert is_fill(rt.tonemap(g), 0xD3, (35, 4), np.uint8)
        assert shim.seen == dict(fb=g.g.frame_buffer, size=(7, 5))
        fails_clean(shim, "rt_tonemap", rt.tonemap, g)
        fails_clean(shim, "rt_download", rt.tonemap, g)
    finally:
        g.free()


def test_checks_made_before_anything_is_allocated_or_copied(shim):
    """what the staging path checks that the wrappers it replaced did not: a guide array that does not match the
    frame is refused before any allocation (it used to be refused after them), and GBuffer.upload refuses an
    array of the wrong size (it used to copy however many bytes the array had).  Unlike the rest of this file,
    this case is expected to fail on the binding as it was before the staging path."""
    f = dref.synthetic_frame(9, 7)
    src, aov_a, cam_a, aov_b, cam_b, _ = rref.case("small_move", 9, 7)
    g, given = _gbuffer((f["fb"], f["sq"], f["count"]), 9, 7), rt.GBuffer(9, 7)
    try:
        raises_unallocated(shim, rt.denoise, g, dict(f, normal=f["normal"][:, :, :2]))
        raises_unallocated(shim, rt.reproject, g, dict(aov_a, depth=aov_a["depth"][1:]), cam_a, aov_b, cam_b)
        raises_unallocated(shim, rt.reproject, g, aov_a, cam_a, dict(aov_b, triangle=aov_b["triangle"][:, 1:]), cam_b,
                           out=given)
        before, shim.calls[:] = g.download(), []
        for fb in (f["fb"][1:], np.concatenate([f["fb"], f["fb"]])):
            with pytest.raises(ValueError):
                g.upload(fb, f["sq"], f["count"], before[3])
        assert "rt_upload" not in shim.calls and all(same_bits(a, b) for a, b in zip(g.download(), before))
    finally:
        g.free()
        given.free()


def test_gbuffer_and_counters_round_trip(shim):
    g = rt.GBuffer(7, 5, seed_skip=3)
    try:
        fb, sq, cnt, rng = g.download()
        assert (fb.shape, sq.shape, cnt.shape, rng.shape) == ((35, 3), (35,), (35,), (35,))
        assert (fb.dtype, sq.dtype, cnt.dtype, rng.dtype) == (F, F, np.int32, np.uint32)
        assert not fb.any() and not sq.any() and not cnt.any() and np.array_equal(rng, rt.seeds(35, 3))
        new = (rays_of(35)[:, :3].copy(), rays_of(35, 4)[:, 0].copy(), np.arange(35, dtype=np.int32), rt.seeds(35, 70))
        g.upload(new[0].reshape(5, 7, 3), new[1].astype(np.float64), new[2].reshape(5, 7), new[3])
        assert all(same_bits(a, b) for a, b in zip(g.download(), new))
    finally:
        g.free()
    c = rt.DeviceCounters()
    assert shim.calls[-2:] == ["rt_device_alloc", "rt_memset"]
    words = np.arange(1, rt.N_COUNTERS + 1, dtype=np.uint64)
    shim.rt_upload(c.p, words.ctypes.data, words.nbytes)
    got = c.read(finisher=True)
    assert [got[k] for k in rt.COUNTER_NAMES] == list(range(1, 11)) and got["deep_push"] == 16
    assert [got[k] for k in rt.FINISH_COUNTER_NAMES] == list(range(11, 41))
    assert set(c.read()) == set(rt.COUNTER_NAMES) | {"deep_push"}
    c.zero()
    assert not any(c.read(finisher=True).values())
    del c
