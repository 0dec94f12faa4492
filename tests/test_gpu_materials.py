"""The kernels' shading across the material space, against the recorded results
of the reference's own source (tests/golden/reference/materials.npz and
materials_nonfinite.npz; cases and scenes: tests/reference_cases.py,
tests/hazards.py).

The BSDF on the device (csrc/rt_kernels.h: scatter, fresnel_*, lambda_,
specular_weight, refraction_direction, the FP64 island of the microfacet
normal) is reachable only through a scene, and four loops consume it:
path_bounce (the megakernel and rt_path_query_kernel), wf_shade.h's shade_step,
the finishers and wf_long.  `materials` puts one box per material extreme in
front of the camera (roughness 0 .. 1.5, n 0.5 .. 100, k 1e-20 .. 50, albedo 0,
2 and 1e-30, emissive glass and metal, values whose squares are f32 denormals)
and is driven through each of those loops; its frames are finite and compared
bit for bit.  `materials_nonfinite` makes NaN and Inf (3e38, 1e30, n = 0) and
is compared by class (helpers.assert_same_class): NaN exactly where the
reference has NaN, every other value bit for bit — through rt_render, wf_long,
chained calls, the path queries with the adaptive test, rt_tonemap and
rt_convergence.  test_gpu_reference.py runs `materials` through rt_render's
four configurations with the other frame cases.
"""
import numpy as np
import pytest

import helpers
import reference_cases as rc
import rt
import test_gpu_deep_bounded as tdb
import test_gpu_parity as tpar
import test_gpu_query as tq
import test_gpu_reference as tr
from test_gpu_reference import workdir  # noqa: F401  (the module's fixture)

pytestmark = pytest.mark.gpu
f32 = np.float32
FINITE, NONFINITE = "materials", "materials_nonfinite"
TRAVERSALS = [pytest.param(rt.TRAVERSAL_KD, id="kd"), pytest.param(rt.TRAVERSAL_BOUNDED, id="bounded")]
MODES = [pytest.param(m, id="bounded" if m == rt.TRAVERSAL_BOUNDED else "kd") for m in tq.MODES]
# the parameter sets of test_gpu_parity's test_wavefront_finisher_modes and test_wavefront_long_paths_and_pipelines
WAVEFRONT_ROUTES = (
    [pytest.param(dict(wf_tail=t, wf_finish_waves=w, wf_wide=wide), id=i)
     for (t, w, wide), i in zip(tpar.FINISHER_MODES, tpar.FINISHER_MODE_IDS)]
    + [pytest.param(dict(wf_long_depth=d, wf_pipelines=p), id=i) for (d, p), i in zip(tpar.LONG_MODES, tpar.LONG_MODE_IDS)])


def render(fx, run, kernel, traversal, **kw):
    """test_gpu_reference.render's frames, its G-buffer freed"""
    got, g = tr.render(fx, run, kernel, traversal, **kw)
    g.free()
    return got


def compare(name, got, want, what):
    (helpers.assert_same_class if name in rc.NONFINITE_CASES else helpers.assert_bitwise)(got, want, what=what)


def final(fx):
    return rc.fixture_frames(fx)[-1]


# ------------------------------------------------------------------ a. the non-finite case through rt_render
@pytest.mark.parametrize("kernel,traversal", tr.CONFIGS)
def test_nonfinite_frames_equal_the_recorded_reference(workdir, kernel, traversal):  # noqa: F811
    """the G-buffer after each call: NaN where the reference has NaN, everything else (Inf, the finite pixels,
    sample_count as the adaptive test left it, random_numbers) bit for bit"""
    fx, run = tr.gpu_case(workdir, NONFINITE)
    got = render(fx, run, kernel, traversal)
    for c, (g, want) in enumerate(zip(got, rc.fixture_frames(fx))):
        helpers.assert_same_class(g, want, what=f"{NONFINITE} call {c} vs the recorded reference:")
    assert np.isnan(final(fx)[0]).any() and np.isinf(final(fx)[0]).any() and len(np.unique(final(fx)[2])) >= 3


# ------------------------------------------------------------------ b. every shading text
@pytest.mark.parametrize("traversal", TRAVERSALS)
@pytest.mark.parametrize("mode", WAVEFRONT_ROUTES)
def test_materials_through_every_wavefront_route(workdir, mode, traversal):  # noqa: F811
    """wf_shade / wf_finish, wf_finish_coop, wf_finish_bvh at every hand-off point and width, wf_long from
    depth 1 and 3, the pipeline split"""
    fx, run = tr.gpu_case(workdir, FINITE)
    got = render(fx, run, rt.KERNEL_WAVEFRONT, traversal, **mode)
    helpers.assert_bitwise(got[-1], final(fx), what=f"{FINITE} {mode} vs the recorded reference:")


@pytest.mark.parametrize("traversal", TRAVERSALS)
@pytest.mark.parametrize("name", [FINITE, NONFINITE])
def test_through_wf_long(workdir, name, traversal):  # noqa: F811
    """paths deeper than 16 bounces finish in wf_long; none of its failure counters moves"""
    fx, run = tr.gpu_case(workdir, name)
    rt.deviation_stats(reset=True)
    got = render(fx, run, rt.KERNEL_WAVEFRONT, traversal, wf_long_depth=16)
    compare(name, got[-1], final(fx), f"{name}, wf_long_depth 16, vs the recorded reference:")
    stats = rt.deviation_stats()
    assert stats["max_deep_depth"] > 16 and all(stats[k] == 0 for k in tdb.FAILURES), stats


@pytest.mark.parametrize("long_depth", [0, 16], ids=["chained", "chained-wf_long-16"])
@pytest.mark.parametrize("name", [FINITE, NONFINITE])
def test_chained_calls(workdir, name, long_depth):  # noqa: F811
    """the case's two calls chained (overlap: the second is queued behind the first, one join at the end)"""
    fx, run = tr.gpu_case(workdir, name)
    assert len(fx["meta"]["passes"]) == 2
    got = render(fx, run, rt.KERNEL_WAVEFRONT, rt.TRAVERSAL_BOUNDED, overlap=True, wf_long_depth=long_depth)
    compare(name, got[-1], final(fx), f"{name} chained, wf_long_depth {long_depth}, vs the recorded reference:")


def test_materials_under_the_guard(workdir):  # noqa: F811
    """check_interval 1: every finisher ray re-traced by the plain KD traversal, none disagrees"""
    fx, run = tr.gpu_case(workdir, FINITE)
    rt.deviation_stats(reset=True)
    got = render(fx, run, rt.KERNEL_WAVEFRONT, rt.TRAVERSAL_BOUNDED, check_interval=1)
    helpers.assert_bitwise(got[-1], final(fx), what=f"{FINITE}, check_interval 1, vs the recorded reference:")
    stats = rt.deviation_stats()
    assert stats["bounded_checked"] > 0 and stats["bounded_mismatches"] == 0, stats


# ------------------------------------------------------------------ c. the path-query loop
def _sampler(fx):
    m = fx["meta"]
    return rt.Sampler("pinhole", m["width"], m["height"], tr._camera(fx["camera"]))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", [FINITE, NONFINITE])
def test_trace_paths_on_the_camera_samples(workdir, name, mode):  # noqa: F811
    """rt_trace_paths on the frame's camera samples (drawn by the sampler's host twin, which
    tests/test_samplers_cpu.py pins to the oracle's camera sample), one accumulating call per pass.  A ray
    list carries no adaptive test, so of the adaptive case the pixels compared after a call are those that ran
    every pass so far"""
    fx, run = tr.gpu_case(workdir, name)
    m = fx["meta"]
    smp, rng, rad, sq, done = _sampler(fx), fx["seeds"], None, None, 0
    for c, (passes, want) in enumerate(zip(m["passes"], rc.fixture_frames(fx))):
        for _ in range(passes):
            rays, st = rt.sampler_rays_host(smp, rng)
            rad, sq, rng = rt.trace_paths(run.dev, rays, st, samples=1, traversal=mode, radiance=rad, sq=sq)
        done += passes
        px = np.nonzero(want[2] == done)[0]
        assert len(px) >= (smp.n if not m["adaptive"] else 100), (name, c, len(px))
        compare(name, (rad[px], sq[px], want[2][px], rng[px]), tuple(a[px] for a in want),
                f"{name} call {c} mode {mode}: rt_trace_paths vs the recorded reference:")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", [FINITE, NONFINITE])
def test_sample_paths_with_the_pinhole_sampler(workdir, name, mode):  # noqa: F811
    """rt_sample_paths (the adaptive case: rt_sample_paths_adaptive with the case's min_samples and tolerance)
    draws the camera samples itself: the case's calls, accumulating, give the recorded G-buffer"""
    fx, run = tr.gpu_case(workdir, name)
    m = fx["meta"]
    adaptive = (m["min_samples"], m["tolerance"]) if m["adaptive"] else None
    smp, rng, rad, sq, cnt = _sampler(fx), fx["seeds"], None, None, True
    for c, (passes, want) in enumerate(zip(m["passes"], rc.fixture_frames(fx))):
        rad, sq, rng, cnt = rt.sample_paths(run.dev, smp, rng, samples=passes, traversal=mode, radiance=rad, sq=sq,
                                            count=cnt, adaptive=adaptive)
        compare(name, (rad, sq, cnt, rng), want,
                f"{name} call {c} mode {mode}: rt_sample_paths vs the recorded reference:")


# ------------------------------------------------------------------ d. consumers of a non-finite frame
def test_tonemap_of_the_nonfinite_frame(workdir):  # noqa: F811
    """rt_tonemap of the recorded final G-buffer with every 7th count 0 (1 / count, 0 * inf, fminf / fmaxf and the
    float-to-byte conversion on NaN and Inf) gives the reference's bytes"""
    fx, _ = tr.gpu_case(workdir, NONFINITE)
    fb, sq, cnt, rng = final(fx)
    g = rt.GBuffer(fx["meta"]["width"], fx["meta"]["height"])
    try:
        g.upload(fb, sq, rc.zeroed_counts(cnt), rng)
        rgba = rt.tonemap(g)
    finally:
        g.free()
    bad = np.nonzero((rgba != fx["tonemap_rgba"]).any(axis=1))[0]
    assert len(bad) == 0, (len(bad), bad[:8], rgba[bad[:3]], fx["tonemap_rgba"][bad[:3]], fb[bad[:3]])


@pytest.mark.parametrize("zeroed", [False, True], ids=["counts", "every-7th-count-0"])
def test_convergence_of_the_nonfinite_frame(workdir, zeroed):  # noqa: F811
    """rt_convergence on the recorded final G-buffer against its host twin: open, below-min and sample counts
    equal, the error map by class"""
    fx, _ = tr.gpu_case(workdir, NONFINITE)
    fb, sq, cnt, _ = final(fx)
    cnt = rc.zeroed_counts(cnt) if zeroed else cnt
    m = fx["meta"]
    got, err = rt.convergence(fb, sq, cnt, m["min_samples"], m["tolerance"], rel_error=True)
    want, want_err = rt.convergence_host(fb, sq, cnt, m["min_samples"], m["tolerance"], rel_error=True)
    assert got == want, (got, want)
    assert 0 < want["open"] < len(cnt), want  # pixels on both sides of the adaptive test
    helpers.assert_same_class((err,), (want_err,), what="rt_convergence's error map vs rt_convergence_host:",
                              names=("rel_error",))
    assert np.isnan(fb).any() and np.isinf(sq).any()  # what the statistic was computed from
