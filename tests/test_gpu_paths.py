"""The radiance query on the GPU (rt_trace_paths; csrc/query.hip
rt_path_query_kernel) against its definition: the reference's trace_path on
the caller's rays, bit for bit.

The reference is never the code under test.  For a ray list that is a frame's
camera samples (path_query_ref.camera_samples, pinned by tests/test_paths_cpu.
py) it is the oracle's or_render: one pass from reset leaves frame_buffer =
+0 + L, squared_luminance = luminance(L)^2 and random_numbers = the state
after the path.  For arbitrary rays and for repeated samples of one ray, which
or_render cannot make, it is the independent scalar restatement
independent_path.Scene.trace_path.  Every comparison is bitwise.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import hazards
import helpers
import independent_path as ip
import oracle
import path_query_ref as pq
import rt
import test_gpu_query as tq

pytestmark = pytest.mark.gpu
f32 = np.float32
MODES = tq.MODES


# ------------------------------------------------------------------ references (no GPU)
_frames = {}


def oracle_frame(path, W, H, max_depth=0, camera=None, key=None):
    """one or_render pass from reset -> ((fb, sq, rng), counters incl. 'cut'); computed once per frame, read-only"""
    key = key or (path, W, H, max_depth)
    if key not in _frames:
        dev = {}
        (fb, sq, cnt, rng), k = helpers.oracle_render(path, W, H, 1, max_depth=max_depth, camera=camera, deviations=dev)
        assert (cnt == 1).all()
        k["cut"] = dev["cut"]
        for a in (fb, sq, rng):
            a.setflags(write=False)
        _frames[key] = ((fb, sq, rng), k)
    return _frames[key]


def frame_rays(camera7, W, H, pixels=None):
    """the frame's first camera samples as a ray list, and the RNG states trace_path starts from"""
    seeds = oracle.mt19937(W * H)
    return pq.camera_samples(camera7, W, H, seeds if pixels is None else seeds[pixels], pixels)


def check_reference_is_not_trivial(ref, k, W, H, what):
    """conditions on the oracle's frame alone: NEE ran, light and dark pixels, and structure"""
    fb = ref[0].reshape(H, W, 3)
    lit = (fb != 0).any(axis=2)
    differs = np.zeros((H, W), bool)
    differs[:, :-1] = (fb[:, :-1] != fb[:, 1:]).any(axis=2)
    print(f"{what}: nee {k['nee']}, lit {lit.mean():.3f}, dark or unlike the neighbour {(~lit | differs).mean():.3f}")
    assert k["nee"] > 0, what
    assert lit.mean() >= 0.10, (what, lit.mean())
    assert (~lit | differs).mean() >= 0.10, what


def assert_stats(st, k, n, samples=1):
    assert st["rays"] == n and st["paths"] == n * samples, st
    assert st["paths"] == k["sample"] and st["trace_calls"] == k["ray"], (st, k)
    assert st["cut_paths"] == k["cut"] and st["max_depth"] == k["maxdepth"], (st, k)


def chain(dev, rays, rng, calls, **kw):
    """a 1-sample call, then calls - 1 accumulating 1-sample calls that feed rng_out back"""
    rad, sq, rng = rt.trace_paths(dev, rays, rng, samples=1, **kw)
    for _ in range(calls - 1):
        rad, sq, rng = rt.trace_paths(dev, rays, rng, samples=1, radiance=rad, sq=sq, **kw)
    return rad, sq, rng


_ip_scenes = {}


def ip_scene(c):
    if c.run.path not in _ip_scenes:
        _ip_scenes[c.run.path] = ip.Scene(c.run.host.triangles_bytes()[0])
    return _ip_scenes[c.run.path]


# ------------------------------------------------------------------ 1. camera samples == the oracle's frame
@pytest.mark.parametrize("name", ["cornell", "room_small"])
def test_camera_samples_equal_the_oracles_frame(name):
    c = tq.case(name)
    W, H = 96, 54
    ref, k = oracle_frame(c.run.path, W, H)
    check_reference_is_not_trivial(ref, k, W, H, name)
    rays, st = frame_rays(c.osc.camera, W, H)
    for mode in MODES:
        rad, sq, rng, stats = rt.trace_paths(c.run.dev, rays, st, traversal=mode, stats=True)
        pq.assert_same((rad, sq, rng), ref, f"{name} mode {mode}")
        assert_stats(stats, k, W * H)


# ------------------------------------------------------------------ 2. samples, accumulation and order
def test_samples_accumulation_and_order():
    c = tq.case("cornell")
    n, S = 1000, 5
    rays = c.rays("inbox")[:n]
    seeds = oracle.mt19937(n, 7)
    one = rt.trace_paths(c.run.dev, rays, seeds, samples=S)
    assert (one[0] != 0).any(axis=1).mean() > 0.25 and (one[2] != seeds).mean() > 0.25
    pq.assert_same(chain(c.run.dev, rays, seeds, S), one, "5 samples in one call vs 1 + 4 accumulating calls")
    m = 48
    want = pq.scalar_paths(ip_scene(c), rays[:m], seeds[:m], samples=S)
    assert (want[0] != 0).any(axis=1).sum() >= 12
    pq.assert_same(tuple(a[:m] for a in one), want, "5 samples vs the scalar trace_path summed in sample order")
    # and the sum is not one sample times 5: the samples differ
    first = rt.trace_paths(c.run.dev, rays[:m], seeds[:m], samples=1)
    assert (one[0][:m] != first[0] * f32(S)).any()


# ------------------------------------------------------------------ 3. arbitrary rays
def arbitrary_rays(c):
    """64 rays: 8 in-box unit, 8 from outside, 8 scaled by 0.25, 8 by 4, 8 axis-parallel, 8 that miss the
    scene, 16 with non-finite, zero, huge or denormal components"""
    lo, hi = c.bounds[:3], c.bounds[3:]
    away = np.concatenate([np.tile(hi + (hi - lo), (8, 1)), tq._unit(np.random.default_rng(5), 8)], axis=1).astype(f32)
    away[:, 3:] = np.abs(away[:, 3:])  # from beyond the box's far corner, pointing further away
    special = c.rays("special")[[0, 3, 6, 9, 12, 16, 20, 28, 36, 40, 48, 52, 54, 56, 60, 63]]
    return np.concatenate([c.rays("inbox")[:8], c.rays("outside")[:8], c.rays("gate:0.25")[:8], c.rays("gate:4")[:8],
                           c.rays("axis")[:8], away, special]).astype(f32)


def test_arbitrary_rays():
    c = tq.case("cornell")
    rays = arbitrary_rays(c)
    assert rays.shape == (64, 6)
    seeds = oracle.mt19937(64, 3)
    want = pq.scalar_paths(ip_scene(c), rays, seeds)
    lit = (want[0] != 0).any(axis=1)
    assert lit[:8].sum() >= 2 and lit[16:32].sum() >= 2, lit  # the unit and the scaled classes carry light
    # the rays that miss, and every ray with a non-finite or zero component: L = 0 and the RNG untouched
    assert not lit[40:48].any() and np.array_equal(want[2][40:48], seeds[40:48])
    nonfinite = ~np.isfinite(rays).all(axis=1)
    zero_dir = (rays[:, 3:] == 0).all(axis=1)
    assert nonfinite.sum() >= 8 and zero_dir.sum() >= 2
    assert not lit[nonfinite | zero_dir].any() and np.array_equal(want[2][nonfinite | zero_dir], seeds[nonfinite | zero_dir])
    # the gate classes, by rt_trace_rays' own accounting on the same rays
    for sl, kd in ((slice(0, 16), 0), (slice(16, 32), 16)):
        _, st = rt.trace_rays(c.run.dev, rays[sl], traversal=rt.TRAVERSAL_BOUNDED, stats=True)
        assert st["kd_rays"] == kd, (sl, st)
    for mode in MODES:
        got = rt.trace_paths(c.run.dev, rays, seeds, traversal=mode)
        pq.assert_same(got, want, f"arbitrary rays mode {mode}")


# ------------------------------------------------------------------ 4. deep paths and regeneration
@pytest.fixture(scope="module")
def trap(tmp_path_factory):
    return helpers.GpuRun(helpers.make_trap_scene(str(tmp_path_factory.mktemp("trap")), 60.0))


def test_deep_paths_and_regeneration(trap):
    W = H = 16
    cam = oracle.OracleScene(trap.path).camera
    ref, k = oracle_frame(trap.path, W, H)
    assert k["maxdepth"] >= 64 and k["cut"] == 0, k  # the scene makes a deep path
    rays, st = frame_rays(cam, W, H)
    rt.deviation_stats(reset=True)
    for mode in MODES:
        rad, sq, rng, stats = rt.trace_paths(trap.dev, rays, st, traversal=mode, stats=True)
        pq.assert_same((rad, sq, rng), ref, f"light guide mode {mode}")
        assert_stats(stats, k, W * H)
        two = rt.trace_paths(trap.dev, rays, st, samples=2, traversal=mode)
        pq.assert_same(two, chain(trap.dev, rays, st, 2, traversal=mode), f"light guide, 2 samples, mode {mode}")
    ref8, k8 = oracle_frame(trap.path, W, H, max_depth=8)
    assert k8["cut"] > 0 and k8["maxdepth"] == 8, k8
    for mode in MODES:
        rad, sq, rng, stats = rt.trace_paths(trap.dev, rays, st, max_depth=8, traversal=mode, stats=True)
        pq.assert_same((rad, sq, rng), ref8, f"light guide max_depth 8 mode {mode}")
        assert_stats(stats, k8, W * H)
    d = rt.deviation_stats(reset=True)  # the query leaves the render's statistics alone
    assert d["deep_paths"] == 0 and d["cut_paths"] == 0 and d["max_deep_depth"] == 0, d


# ------------------------------------------------------------------ 5. shapes and untouched surroundings
OFF, PAD = 5, 131


def run_guarded(dev, rays, rng, mode, samples=1, accumulate=None, with_sq=True):
    """rt_trace_paths_device on buffers that sit OFF records into allocations filled with 0xA5; returns the
    results and asserts that nothing outside [0, n) changed and that the rays were not written"""
    n = len(rays)

    def guarded(values, width, dtype):
        a = np.frombuffer(bytes([0xA5]) * ((OFF + n + PAD) * width * 4), dtype=dtype).copy()
        if values is not None:
            a[OFF * width:(OFF + n) * width] = np.asarray(values, dtype).reshape(-1)
        return a

    h_rad = guarded(accumulate[0] if accumulate else None, 3, f32)
    h_sq = guarded(accumulate[1] if accumulate else None, 1, f32)
    h_rng = guarded(rng, 1, np.uint32)
    d_rays, d_rad, d_sq, d_rng = tq.Dev(rays), tq.Dev(h_rad), tq.Dev(h_sq), tq.Dev(h_rng)
    d_stats = tq.Dev(np.zeros(5, np.uint64))
    try:
        rt.trace_paths_device(dev, d_rays.p, d_rng.p.value + 4 * OFF, n, d_rad.p.value + 12 * OFF,
                              d_sq.p.value + 4 * OFF if with_sq else None, samples=samples,
                              accumulate=accumulate is not None, traversal=mode, stats_ptr=d_stats.p)
        rad, sq, out, stats = d_rad.read(), d_sq.read(), d_rng.read(), d_stats.read()
        assert np.array_equal(d_rays.read().view(np.uint32), np.ascontiguousarray(rays).view(np.uint32)), "rays written"
    finally:
        for d in (d_rays, d_rad, d_sq, d_rng, d_stats):
            d.free()
    for a, b, w in ((rad, h_rad, 3), (sq, h_sq, 1), (out, h_rng, 1)):
        lo, hi = OFF * w, (OFF + n) * w
        assert np.array_equal(a[:lo].view(np.uint32), b[:lo].view(np.uint32)), "records before the first written"
        assert np.array_equal(a[hi:].view(np.uint32), b[hi:].view(np.uint32)), "records past the n-th written"
    if not with_sq:
        assert np.array_equal(sq.view(np.uint32), h_sq.view(np.uint32)), "sq written though NULL"
    assert int(stats[0]) == n and int(stats[1]) == n * samples, stats
    return rad[OFF * 3:(OFF + n) * 3].reshape(n, 3), sq[OFF:OFF + n], out[OFF:OFF + n]


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_shapes_and_untouched_surroundings(n):
    """every n around the wave and block sizes: the camera samples of n pixels spread over test 1's frame — one
    sample against the oracle, three against the chaining rule — inside guard records"""
    c = tq.case("cornell")
    W, H = 96, 54
    ref, _ = oracle_frame(c.run.path, W, H)
    pixels = (np.arange(n) * 19 + 7) % (W * H)  # (19 is coprime to 96 * 54: no pixel twice)
    rays, st = frame_rays(c.osc.camera, W, H, pixels)
    rays = rays.reshape(n, 6)
    want = tuple(a[pixels] for a in ref)
    for mode in MODES:
        one = run_guarded(c.run.dev, rays, st, mode)
        pq.assert_same(one, want, f"n = {n} mode {mode}")
        no_sq = run_guarded(c.run.dev, rays, st, mode, with_sq=False)
        pq.assert_same((no_sq[0], one[1], no_sq[2]), want, f"n = {n} mode {mode}, sq NULL")
        three = run_guarded(c.run.dev, rays, st, mode, samples=3)
        acc = one
        for _ in range(2):
            acc = run_guarded(c.run.dev, rays, acc[2], mode, accumulate=(acc[0], acc[1]))
        pq.assert_same(three, acc, f"n = {n} mode {mode}: 3 samples vs the chain")
        if n >= 63:
            assert (three[0] != one[0]).any()


def test_more_rays_than_resident_lanes():
    """n = 300,000, a 600 x 500 frame's camera samples: more rays than the resident grid has lanes, so every
    lane takes new rays many times"""
    c = tq.case("cornell")
    W, H = 600, 500
    ref, k = oracle_frame(c.run.path, W, H)
    rays, st = frame_rays(c.osc.camera, W, H)
    got = run_guarded(c.run.dev, rays, st, rt.TRAVERSAL_BOUNDED)
    pq.assert_same(got, ref, "600 x 500 camera samples")
    assert (ref[0] != 0).any(axis=1).mean() > 0.10 and k["nee"] > 0


# ------------------------------------------------------------------ 6. hazard geometry
@pytest.mark.parametrize("variant", ["degenerate", "duplicate", "aligned"])
def test_hazard_geometry(tmp_path, variant):
    """zero-area triangles, a duplicated quad (two passing tests at the same s), and the axis-aligned room
    whose walls lie in KD split planes"""
    extra = {"degenerate": hazards.DEGENERATE_OBJ, "duplicate": hazards.DUPLICATE_OBJ, "aligned": ""}[variant]
    path = hazards.cornell_variant(str(tmp_path / variant), variant, yaw_room=0.0 if variant == "aligned" else 0.1,
                                   extra_obj=extra)
    run = helpers.GpuRun(path)
    W, H = 64, 36
    ref, k = oracle_frame(path, W, H)
    check_reference_is_not_trivial(ref, k, W, H, variant)
    rays, st = frame_rays(oracle.OracleScene(path).camera, W, H)
    for mode in MODES:
        rad, sq, rng, stats = rt.trace_paths(run.dev, rays, st, traversal=mode, stats=True)
        pq.assert_same((rad, sq, rng), ref, f"{variant} mode {mode}")
        assert_stats(stats, k, W * H)


# ------------------------------------------------------------------ 7. textured scene
def test_textured_scene(tmp_path):
    scene, files = helpers.make_textured_scene(str(tmp_path))
    for rel in files:
        oracle.register_texture(rel, rt.decode_image(os.path.join(str(tmp_path), rel)))
    run = helpers.GpuRun(scene)
    W, H = 48, 27
    ref, k = oracle_frame(scene, W, H)
    assert k["texel"] > 0 and k["nee"] > 0 and (ref[0] != 0).any(axis=1).mean() > 0.10, k
    rays, st = frame_rays(oracle.OracleScene(scene).camera, W, H)
    for mode in MODES:
        pq.assert_same(rt.trace_paths(run.dev, rays, st, traversal=mode), ref, f"textured room mode {mode}")


# ------------------------------------------------------------------ 8. between chained renders
def test_trace_paths_between_chained_renders():
    """two chained rt_render calls (overlap = 1) with an rt_trace_paths on another stream between them: the
    frame is the one without the query, and the query's outputs are the standalone ones"""
    c = tq.case("room_small")
    W, H, P = 96, 54, 4
    qref, _ = oracle_frame(c.run.path, W, H)
    rays, st = frame_rays(c.osc.camera, W, H)
    n = W * H
    alone = rt.trace_paths(c.run.dev, rays, st)
    pq.assert_same(alone, qref, "standalone")
    s_render, s_query = tq._stream(), tq._stream()

    def frame(with_query):
        gb = rt.GBuffer(W, H)
        d_rays, d_rng = tq.Dev(rays), tq.Dev(np.concatenate([st, np.full(64, 0xA5A5A5A5, np.uint32)]))
        d_rad, d_sq = tq.Dev(np.full(3 * n + 64, -7.0, f32)), tq.Dev(np.full(n + 64, -7.0, f32))
        try:
            for k in range(2):
                opt = rt.options(W, H, P, adaptive=False, kernel=rt.KERNEL_WAVEFRONT, overlap=True,
                                 coalesce_passes=-1, stream=s_render.value)
                rt.render(c.run.dev, gb, c.run.camera, 0 if k == 0 else 1, opt)
                if with_query and k == 0:
                    rt.trace_paths_device(c.run.dev, d_rays.p, d_rng.p, n, d_rad.p, d_sq.p, stream=s_query.value)
            rt.join()
            assert tq._HIP.hipStreamSynchronize(s_query) == 0
            return gb.download(), d_rad.read(), d_sq.read(), d_rng.read()
        finally:
            for d in (d_rays, d_rng, d_rad, d_sq):
                d.free()
            gb.free()

    plain = frame(False)[0]
    mixed, rad, sq, rng = frame(True)
    helpers.assert_bitwise(mixed, plain, what="chained frame with a radiance query in between")
    assert int(plain[2].sum()) == W * H * P * 2
    pq.assert_same((rad[:3 * n].reshape(n, 3), sq[:n], rng[:n]), alone, "the query between chained renders")
    assert (rad[3 * n:] == f32(-7.0)).all() and (sq[n:] == f32(-7.0)).all() and (rng[n:] == 0xA5A5A5A5).all()
    for s in (s_render, s_query):
        assert tq._HIP.hipStreamDestroy(s) == 0


# ------------------------------------------------------------------ 9. torch
def test_torch_tensors_on_the_current_stream():
    """rays, rng and the outputs in torch device tensors, the query enqueued on torch's current stream
    (rt.trace_paths_device): the numpy path's results.  In a child process that imports torch first
    (tests/paths_torch_child.py)."""
    pytest.importorskip("torch")
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "paths_torch_child.py")
    r = subprocess.run([sys.executable, child], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout[-2000:] + r.stderr[-4000:]
