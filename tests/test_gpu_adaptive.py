"""rt_sample_paths_adaptive and rt_convergence on the GPU, bit for bit:

1. a PINHOLE sampler on a G_Buffer's four arrays is rt_render with the adaptive test on — against the oracle's
   adaptive frame and against rt_render on both kernels, in one call, in calls of 6 + 10 samples, at min_samples 1
   and 0;
2. every kind (pixel lists with entries outside the frame, hemisphere points) equals the host-driven loop of
   { open set by rt_convergence_host; rt_sample_paths(samples = 1, accumulate = 1) on the gathered sub-problem;
   scatter }, inside guard words;
3. an all-converged call samples nothing and changes no byte; rt_convergence equals rt_convergence_host, also after
   chained renders that nobody joined;
4. the driver's --until-converged and --error-map.

The references are the oracle, rt_render and the non-adaptive calls — never the code under test."""
import subprocess

import numpy as np
import pytest

import helpers
import oracle
import rt
import test_adaptive_cpu as ac
import test_gpu_query as tq
import test_gpu_samplers as ts

pytestmark = pytest.mark.gpu
f32 = np.float32
MODES = tq.MODES
W, H, PASSES, MIN_SAMPLES, TOLERANCE = ac.W, ac.H, ac.PASSES, ac.MIN_SAMPLES, ac.TOLERANCE
N = W * H
OFF = ts.OFF


def adaptive_frame(c, smp, samples, mode, adaptive, gb=None, accumulate=False):
    """rt_sample_paths_adaptive on a G_Buffer's four arrays -> (fb, sq, count, rng), and the call's stats"""
    own = gb is None
    gb = gb or rt.GBuffer(smp.width, smp.height)
    d_stats = tq.Dev(np.zeros(5, np.uint64))
    try:
        rt.sample_paths_device(c.run.dev, smp, gb.g.random_numbers, gb.n, gb.g.frame_buffer, gb.g.squared_luminance,
                               gb.g.sample_count, samples=samples, accumulate=accumulate, traversal=mode,
                               stats_ptr=d_stats.p, adaptive=adaptive)
        return gb.download(), dict(zip(rt.PATH_STATS, (int(v) for v in d_stats.read())))
    finally:
        d_stats.free()
        if own:
            gb.free()


def open_mask(rad, sq, cnt, min_samples, tolerance):
    """rt_convergence_host's `open`, asked of every element alone"""
    return np.array([rt.convergence_host(rad[i], sq[i:i + 1], cnt[i:i + 1], min_samples, tolerance)["open"]
                     for i in range(len(cnt))], dtype=bool)


# ------------------------------------------------------------------ 1. the pinhole sampler is adaptive rt_render
@pytest.mark.parametrize("name", ["cornell", "room_small"])
def test_pinhole_equals_the_oracle_and_rt_render(name):
    c = tq.case(name)
    smp = ts.image_sampler(c, "pinhole")
    fb, sq, cnt, rng, _ = ac.oracle_frame(name)
    ref = (fb, sq, cnt, rng)
    test = (MIN_SAMPLES, TOLERANCE)
    kw = dict(adaptive=True, min_samples=MIN_SAMPLES, tolerance=TOLERANCE)
    renders = {k: c.run.render(W, H, PASSES, kernel=k, **kw)[0] for k in (rt.KERNEL_MEGA, rt.KERNEL_WAVEFRONT)}
    for k, frame in renders.items():
        helpers.assert_bitwise(frame, ref, what=f"{name}: rt_render kernel {k} vs the oracle")
    for mode in MODES:
        got, stats = adaptive_frame(c, smp, PASSES, mode, test)
        helpers.assert_bitwise(got, ref, what=f"{name} mode {mode}: {PASSES} adaptive samples vs the oracle")
        for k, frame in renders.items():
            helpers.assert_bitwise(got, frame, what=f"{name} mode {mode}: vs rt_render kernel {k}")
        assert stats["rays"] == N and stats["paths"] == int(got[2].sum()) < PASSES * N
        # in calls of 6 + 10 samples
        gb = rt.GBuffer(W, H)
        try:
            _, s1 = adaptive_frame(c, smp, 6, mode, test, gb)
            got, s2 = adaptive_frame(c, smp, 10, mode, test, gb, accumulate=True)
        finally:
            gb.free()
        helpers.assert_bitwise(got, ref, what=f"{name} mode {mode}: 6 + 10 adaptive samples vs the oracle")
        assert s1["paths"] + s2["paths"] == int(got[2].sum())
    split = c.run.render(W, H, [6, 10], kernel=rt.KERNEL_WAVEFRONT, **kw)[0]
    helpers.assert_bitwise(split, ref, what=f"{name}: rt_render in calls of 6 + 10 passes vs the oracle")


@pytest.mark.parametrize("min_samples", [1, 0])
def test_pinhole_min_samples_1_and_0(min_samples):
    """the variance divides by count - 1: at min_samples 1 a pixel's second test divides by 0; at 0 its first is
    0 / 0, which fails the compare — nothing is sampled and the RNG stays"""
    c = tq.case("cornell")
    smp = ts.image_sampler(c, "pinhole")
    kw = dict(adaptive=True, min_samples=min_samples, tolerance=TOLERANCE)
    renders = [c.run.render(W, H, PASSES, kernel=k, **kw)[0] for k in (rt.KERNEL_MEGA, rt.KERNEL_WAVEFRONT)]
    helpers.assert_bitwise(renders[0], renders[1], what="rt_render: the two kernels")
    for mode in MODES:
        got, stats = adaptive_frame(c, smp, PASSES, mode, (min_samples, TOLERANCE))
        helpers.assert_bitwise(got, renders[1], what=f"min_samples {min_samples} mode {mode} vs rt_render")
        assert stats["paths"] == int(got[2].sum()) and stats["rays"] == N
        if min_samples == 0:
            assert stats["paths"] == 0 and stats["trace_calls"] == 0
            assert (got[2] == 0).all() and not got[0].any() and not got[1].any()
            assert np.array_equal(got[3], oracle.mt19937(N))
        else:
            assert 0 < stats["paths"] < PASSES * N and got[2].min() >= 1


# ------------------------------------------------------------------ 2. every kind equals the host-driven loop
def sub_sampler(smp, idx):
    if smp.points is not None:
        return rt.Sampler("hemisphere", points=smp.points[idx])
    return rt.Sampler(smp.kind, smp.width, smp.height, smp.camera, ortho_half_width=smp.ortho_half_width,
                      pixels=smp.pixels[idx])


def host_driven(c, smp, st, rounds, test, mode):
    n = smp.n
    rad, sq, cnt, rng = np.zeros((n, 3), f32), np.zeros(n, f32), np.zeros(n, np.int32), st.copy()
    taken = 0
    for _ in range(rounds):
        idx = np.nonzero(open_mask(rad, sq, cnt, *test))[0]
        if not len(idx):
            break
        r, s, g, k = rt.sample_paths(c.run.dev, sub_sampler(smp, idx), rng[idx], samples=1, traversal=mode,
                                     radiance=rad[idx], sq=sq[idx], count=cnt[idx])
        rad[idx], sq[idx], rng[idx], cnt[idx] = r, s, g, k
        taken += len(idx)
    return (rad, sq, cnt, rng), taken


def fused_guarded(c, smp, st, samples, test, mode):
    """rt_sample_paths_adaptive on buffers inside guard words; the pixel list / points sit in exact-size buffers"""
    n = smp.n
    host = [ts.guarded(None, n, 3, f32), ts.guarded(None, n, 1, f32), ts.guarded(None, n, 1, np.int32),
            ts.guarded(st, n, 1, np.uint32)]
    dev = [tq.Dev(a) for a in host]
    d_pix = tq.Dev(smp.pixels) if smp.pixels is not None else None
    d_pts = tq.Dev(smp.points) if smp.points is not None else None
    d_stats = tq.Dev(np.zeros(5, np.uint64))
    try:
        rad, sq, cnt, rng = (d.p.value + 4 * OFF * w for d, w in zip(dev, (3, 1, 1, 1)))
        rt.sample_paths_device(c.run.dev, smp, rng, n, rad, sq, cnt, samples=samples, traversal=mode,
                               stats_ptr=d_stats.p, pixels_ptr=d_pix.p if d_pix else None,
                               points_ptr=d_pts.p if d_pts else None, adaptive=test)
        out = [ts.assert_guards(d.read(), h, n, w, what) for d, h, w, what in
               zip(dev, host, (3, 1, 1, 1), ("radiance", "sq", "count", "rng"))]
        out[0] = out[0].reshape(n, 3)
        return tuple(out), dict(zip(rt.PATH_STATS, (int(v) for v in d_stats.read())))
    finally:
        for d in dev + [d_pix, d_pts, d_stats]:
            if d:
                d.free()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("kind", ts.IMAGE + ["hemisphere"])
def test_every_kind_equals_the_host_driven_loop(kind, n):
    c = tq.case("cornell")
    smp = ts.make_sampler(c, kind, n)
    if kind != "hemisphere" and n >= 63:  # entries outside the frame among them
        smp.pixels[[3, 10, 40, 62]] = [-1, W * H, np.iinfo(np.int32).min, np.iinfo(np.int32).max]
    st = oracle.mt19937(n, skip=13)
    test = (2, TOLERANCE)
    want, taken = host_driven(c, smp, st, 8, test, MODES[0])
    for mode in MODES:
        got, stats = fused_guarded(c, smp, st, 8, test, mode)
        helpers.assert_bitwise(got, want, what=f"{kind} n {n} mode {mode}: 8 fused adaptive samples vs 8 host rounds")
        assert stats["rays"] == n and stats["paths"] == taken == int(got[2].sum())
    assert want[2].min() >= 2 and want[2].max() <= 8
    if n >= 63:  # some elements stopped early, some never: the loop had real sub-problems
        assert (want[2] < 8).any() and (want[2] == 8).any(), np.bincount(want[2])
        if kind != "hemisphere":  # the entries outside the frame hit nothing and stop at min_samples
            out = [3, 10, 40, 62]
            assert (want[2][out] == 2).all() and not want[0][out].any() and np.array_equal(want[3][out], st[out])


def test_no_elements_no_launch():
    c = tq.case("cornell")
    smp = ts.make_sampler(c, "equirect", 0)
    rad, sq, rng, cnt = rt.sample_paths(c.run.dev, smp, np.zeros(0, np.uint32), samples=8, adaptive=(2, TOLERANCE))
    assert rad.shape == (0, 3) and len(sq) == len(rng) == len(cnt) == 0
    assert rt.convergence(np.zeros((0, 3), f32), np.zeros(0, f32), np.zeros(0, np.int32), 2, TOLERANCE) == \
        dict(zip(rt.CONVERGENCE_STATS, (0, 0, 0, 0)))


# ------------------------------------------------------------------ 3. convergence
def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_all_converged_call_samples_nothing():
    """the same call again, accumulating, under a tolerance nothing exceeds: no sample, no ray, no byte changed"""
    c = tq.case("cornell")
    smp = ts.image_sampler(c, "equirect")
    gb = rt.GBuffer(W, H)
    try:
        first, s1 = adaptive_frame(c, smp, PASSES, MODES[0], (MIN_SAMPLES, TOLERANCE), gb)
        assert first[2].min() >= MIN_SAMPLES and s1["paths"] == int(first[2].sum()) < PASSES * N
        assert rt.convergence(first[0], first[1], first[2], MIN_SAMPLES, 1e9)["open"] == 0
        for mode in MODES:
            again, s2 = adaptive_frame(c, smp, PASSES, mode, (MIN_SAMPLES, 1e9), gb, accumulate=True)
            assert s2["rays"] == N and s2["paths"] == 0 and s2["trace_calls"] == 0 and s2["cut_paths"] == 0
            helpers.assert_bitwise(again, first, what=f"mode {mode}: an all-converged call")
    finally:
        gb.free()


_conv = {}


@pytest.mark.parametrize("n", [0, 1, 63, 65, N])
def test_convergence_equals_the_host(n):
    c = tq.case("room_small")
    key = "frame"
    if key not in _conv:
        _conv[key] = adaptive_frame(c, ts.image_sampler(c, "equirect"), PASSES, MODES[0], (MIN_SAMPLES, TOLERANCE))[0]
    fb, sq, cnt, _ = _conv[key]
    for test in ((MIN_SAMPLES, TOLERANCE), (PASSES, 0.05), (0, 0.9), (MIN_SAMPLES, 0.05)):
        want, want_err = rt.convergence_host(fb[:n], sq[:n], cnt[:n], *test, rel_error=True)
        got, err = rt.convergence(fb[:n], sq[:n], cnt[:n], *test, rel_error=True)
        assert got == want, (n, test)
        assert same_bits(err, want_err), (n, test)
        assert rt.convergence(fb[:n], sq[:n], cnt[:n], *test) == want
    if n == N:  # (the last test: a tolerance the frame was not rendered to leaves a real open set)
        print("open under", test, want)
        assert 0 < want["open"] < n and want["below_min"] == 0 and np.isfinite(want_err).any()
    # on device memory, the map inside guard words, the stats added to what the words hold
    h_err = ts.guarded(None, n, 1, f32)
    d_err, d_st = tq.Dev(h_err), tq.Dev(np.array([5, 6, 7, 8], np.uint64))
    dev = [tq.Dev(a[:n]) for a in (fb, sq, cnt)]
    try:
        rt.convergence_device(dev[0].p, dev[1].p, dev[2].p, n, MIN_SAMPLES, TOLERANCE, d_err.p.value + 4 * OFF, d_st.p)
        want, want_err = rt.convergence_host(fb[:n], sq[:n], cnt[:n], MIN_SAMPLES, TOLERANCE, rel_error=True)
        assert same_bits(ts.assert_guards(d_err.read(), h_err, n, 1, "rel_error"), want_err)
        assert [int(v) for v in d_st.read()] == [5 + want["elements"], 6 + want["open"], 7 + want["below_min"],
                                                 8 + want["samples"]]
    finally:
        for d in dev + [d_err, d_st]:
            d.free()


def test_convergence_joins_chained_renders():
    """two chained rt_render calls (overlap = 1) and rt_convergence on their stream, without an rt_join: the
    answer is the finished frame's"""
    c = tq.case("room_small")
    stream = tq._stream()
    gb = rt.GBuffer(W, H)
    d_err, d_st = tq.Dev(np.zeros(N, f32)), tq.Dev(np.zeros(4, np.uint64))
    try:
        for k in range(2):
            opt = rt.options(W, H, 4, adaptive=False, kernel=rt.KERNEL_WAVEFRONT, overlap=True, coalesce_passes=-1,
                             stream=stream.value)
            rt.render(c.run.dev, gb, c.run.camera, 0 if k == 0 else 1, opt)
        rt.convergence_device(gb.g.frame_buffer, gb.g.squared_luminance, gb.g.sample_count, N, MIN_SAMPLES, TOLERANCE,
                              d_err.p, d_st.p, stream=stream.value)
        assert tq._HIP.hipStreamSynchronize(stream) == 0
        err, st = d_err.read(), [int(v) for v in d_st.read()]
        fb, sq, cnt, _ = gb.download()
    finally:
        d_err.free()
        d_st.free()
        gb.free()
        assert tq._HIP.hipStreamDestroy(stream) == 0
    assert (cnt == 8).all()
    want, want_err = rt.convergence_host(fb, sq, cnt, MIN_SAMPLES, TOLERANCE, rel_error=True)
    assert st == [want[k] for k in rt.CONVERGENCE_STATS] and same_bits(err, want_err)
    assert 0 < want["open"] < N and want["samples"] == 8 * N


# ------------------------------------------------------------------ 4. the driver
def drive(args, tmp_path, name, scene="cornell"):
    out = tmp_path / name
    r = subprocess.run([ts.APP, "--scene", helpers.scene_path(scene), "--width", str(W), "--height", str(H), "--quiet",
                        "--out", str(out)] + args, capture_output=True, text=True, timeout=150)
    return r, out


def test_driver_until_converged(tmp_path):
    fixed, f_out = drive(["--adaptive", "0", "--spp", "4"], tmp_path, "fixed.png")
    assert fixed.returncode == 0, fixed.stderr
    stop = ["--until-converged", "--min-samples", "4", "--tolerance", "1e9", "--spp", "64", "--passes", "4"]
    for extra in ([], ["--camera-model", "pinhole"]):
        r, out = drive(stop + extra, tmp_path, "stop%d.png" % len(extra))
        assert r.returncode == 0, r.stderr
        assert f"converged after 4 passes: {4 * N} samples (mean 4.00 per pixel)" in r.stdout, r.stdout
        assert "x 4 passes in" in r.stdout
        assert out.read_bytes() == f_out.read_bytes()
    test = ["--spp", "16", "--min-samples", "4", "--tolerance", "0.3"]
    full, a_out = drive(["--adaptive", "1"] + test, tmp_path, "adaptive.png")
    assert full.returncode == 0, full.stderr
    for extra in ([], ["--passes", "5"], ["--camera-model", "pinhole", "--passes", "5"]):
        r, out = drive(["--until-converged"] + test + extra, tmp_path, "until%d.png" % len(extra))
        assert r.returncode == 0, r.stderr
        assert "not converged: " in r.stdout or "converged after " in r.stdout, r.stdout
        assert out.read_bytes() == a_out.read_bytes(), extra


def test_driver_equirect_until_converged_and_error_map(tmp_path):
    pfm = tmp_path / "err.pfm"
    ckpt = tmp_path / "g.ckpt"
    r, out = drive(["--camera-model", "equirect", "--until-converged", "--spp", "16", "--min-samples", "4", "--tolerance",
                    "0.3", "--passes", "8", "--error-map", str(pfm), "--checkpoint", str(ckpt)], tmp_path, "eq.png",
                   scene="room_small")
    assert r.returncode == 0, r.stderr
    assert "not converged: " in r.stdout or "converged after " in r.stdout, r.stdout
    assert rt.decode_image(str(out)).shape == (H, W, 4)
    err = tq._read_pfm(str(pfm))
    assert err.shape == (H, W) and np.isfinite(err).all() and (err >= 0).all() and (err > 0).mean() > 0.1
    # the map is rt_convergence_host's of the checkpointed frame
    gb = rt.GBuffer(W, H)
    try:
        passes = gb.load(ckpt)
        fb, sq, cnt, _ = gb.download()
    finally:
        gb.free()
    assert passes in (8, 16) and cnt.min() >= 4 and cnt.max() <= passes
    _, want = rt.convergence_host(fb, sq, cnt, 4, 0.3, rel_error=True)
    assert same_bits(np.ascontiguousarray(err.reshape(-1)), want)
    # a plain frame's map: --error-map alone
    r, _ = drive(["--adaptive", "0", "--spp", "1", "--error-map", str(pfm)], tmp_path, "one.png")
    assert r.returncode == 0, r.stderr
    assert np.isposinf(tq._read_pfm(str(pfm))).all()  # one sample per pixel: no variance yet


@pytest.mark.parametrize("args", [
    ["--until-converged", "--adaptive", "0"],
    ["--until-converged", "--shard", "0", "2"],
    ["--until-converged", "--reproject-to", "0 1 0 0 0"],
    ["--until-converged", "--camera-model", "equirect", "--shard", "0", "2"],
    ["--until-converged", "--camera-model", "pinhole", "--adaptive", "1"],
    ["--until-converged", "--min-samples", "-1"],
    ["--error-map"],
])
def test_driver_usage_errors(tmp_path, args):
    r, out = drive(["--spp", "4"] + args, tmp_path, "never.png")
    assert r.returncode == 2 and "usage: rt_render" in r.stderr and not out.exists()
