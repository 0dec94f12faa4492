"""The kernels against the recorded results of the reference's own source.

tests/golden/reference/ holds what the reference (compiled as host C++ by
oracle/Makefile.ref: IEEE arithmetic without contraction, the project's
transcendentals) computed for the cases of tests/reference_cases.py.  Every
other GPU test compares a kernel with the oracle, the project's restatement of
the reference; these compare with the reference's record itself, so a
misreading that the oracle and the kernels share cannot hide.  Only the
fixtures are read: no copy of the reference is needed.

Each case's scene is rebuilt here by the project's scene builders; a SHA-256
of every input file in the fixture tells a drift of those builders from a
kernel bug.
"""
import ctypes

import numpy as np
import pytest

import helpers
import oracle
import reference
import reference_cases as rc
import rt

pytestmark = pytest.mark.gpu
CONFIGS = [pytest.param(k, t, id=f"{kn}-{tn}")
           for k, kn in ((rt.KERNEL_MEGA, "mega"), (rt.KERNEL_WAVEFRONT, "wavefront"))
           for t, tn in ((rt.TRAVERSAL_KD, "kd"), (rt.TRAVERSAL_BOUNDED, "bounded"))]
_cases = {}


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return tmp_path_factory.mktemp("gpu_reference_cases")


def gpu_case(workdir, name):
    """(fixture, scene on the device) of one case, its inputs rebuilt and checked against the fixture's hashes"""
    if name not in _cases:
        fx = rc.load_fixture(name)
        d = workdir / name
        d.mkdir(exist_ok=True)
        case = rc.Case(name, str(d), oracle.OracleScene)
        assert rc.file_hashes(case.path) == fx["meta"]["files"], \
            "the scene's input files drifted from the recorded ones: regenerate tests/golden/reference"
        _cases[name] = (fx, helpers.GpuRun(case.path))
    return _cases[name]


def _camera(arr):
    c = rt.Camera()
    c.position.x, c.position.y, c.position.z = float(arr[0]), float(arr[1]), float(arr[2])
    c.yaw, c.pitch, c.FOV, c.aperture_radius = float(arr[3]), float(arr[4]), float(arr[5]), float(arr[6])
    return c


def render(fx, run, kernel, traversal, **kw):
    """the fixture's calls through rt_render on the fixture's seeds -> the G-buffer after each call"""
    m = fx["meta"]
    W, H = m["width"], m["height"]
    n = W * H
    g = rt.GBuffer(W, H)
    g.upload(np.zeros((n, 3), np.float32), np.zeros(n, np.float32), np.zeros(n, np.int32), fx["seeds"])
    cam = _camera(fx["camera"])
    out = []
    for c, passes in enumerate(m["passes"]):
        rt.render(run.dev, g, cam, 0 if c == 0 else 1,
                  rt.options(W, H, passes, adaptive=m["adaptive"], min_samples=m["min_samples"],
                             tolerance=m["tolerance"], kernel=kernel, traversal=traversal, **kw))
        if not kw.get("overlap"):
            out.append(g.download())
    rt.join()  # chained calls: their deep-path tails
    if kw.get("overlap"):
        out.append(g.download())
    return out, g


@pytest.mark.parametrize("kernel,traversal", CONFIGS)
@pytest.mark.parametrize("name", list(rc.FRAME_CASES))
def test_frames_equal_the_recorded_reference(workdir, name, kernel, traversal):
    """frame_buffer, squared_luminance, sample_count and random_numbers after each call, bit for bit"""
    fx, run = gpu_case(workdir, name)
    got, _ = render(fx, run, kernel, traversal)
    for c, (g, want) in enumerate(zip(got, rc.fixture_frames(fx))):
        helpers.assert_bitwise(g, want, what=f"{name} call {c} vs the recorded reference:")
    if fx["meta"]["adaptive"]:  # the adaptive test really stopped pixels at different counts
        counts = rc.fixture_frames(fx)[-1][2]
        assert counts.min() == fx["meta"]["min_samples"] and counts.max() == sum(fx["meta"]["passes"])


@pytest.mark.parametrize("kernel,traversal", CONFIGS)
def test_chained_calls_equal_the_recorded_reference(workdir, kernel, traversal):
    """the two-call case chained (overlap: the second call is queued behind the first, one join at the end)"""
    fx, run = gpu_case(workdir, "cornell")
    assert len(fx["meta"]["passes"]) == 2
    got, _ = render(fx, run, kernel, traversal, overlap=True)
    helpers.assert_bitwise(got[-1], rc.fixture_frames(fx)[-1], what="cornell chained vs the recorded reference:")


@pytest.mark.parametrize("traversal", [pytest.param(rt.TRAVERSAL_KD, id="kd"),
                                       pytest.param(rt.TRAVERSAL_BOUNDED, id="bounded")])
def test_trap_through_wf_long_equals_the_recorded_reference(workdir, traversal):
    """the trap's deep paths (419 bounces when recorded) handed to wf_long at the smallest depth it takes"""
    fx, run = gpu_case(workdir, "trap")
    rt.deviation_stats(reset=True)
    got, _ = render(fx, run, rt.KERNEL_WAVEFRONT, traversal, wf_long_depth=16)
    helpers.assert_bitwise(got[-1], rc.fixture_frames(fx)[-1], what="trap, wf_long_depth 16, vs the recorded reference:")
    stats = rt.deviation_stats()
    assert stats["max_deep_depth"] >= rc.TRAP_MIN_DEPTH and sum(stats["deep_hist"][2:]) > 0, stats


@pytest.mark.parametrize("name", list(rc.FRAME_CASES))
def test_uploaded_scene_equals_the_recorded_reference(workdir, name):
    """what rt_create_scene uploaded — triangles, KD nodes, indices, the light list (which the product makes
    only here) and the bounds — against the reference's recorded scene"""
    fx, run = gpu_case(workdir, name)
    sc, want = run.dev.scene, fx["meta"]["scene"]
    nt, nn, ni, nl = want["counts"]
    assert (sc.triangle_count, run.dev.node_count, run.dev.index_count, sc.light_count) == (nt, nn, ni, nl)

    def download(ptr, nbytes):
        a = np.zeros(max(nbytes, 1), np.uint8)
        if nbytes:
            rt.check(rt.lib().rt_download(ctypes.c_void_p(a.ctypes.data), ctypes.c_void_p(ptr), nbytes))
        return a[:nbytes]

    lights = download(sc.light_indicies, 4 * nl).view(np.int32)
    np.testing.assert_array_equal(lights, fx["lights"])
    b = sc.kd_tree.bounding_box
    bounds = np.array([b.min.x, b.min.y, b.min.z, b.max.x, b.max.y, b.max.z], np.float32)
    assert bounds.tobytes() == fx["bounds"].tobytes()

    class _Uploaded:  # the device copies with the host's texels (device texel pointers cannot be followed here)
        def arrays(self):
            host = np.frombuffer(run.host.triangles_bytes()[0], np.uint8).reshape(-1, 152)
            tris = download(sc.triangles, 152 * nt).reshape(-1, 152).copy()
            dev_ptr = tris[:, 136:144].copy().view(np.uint64)[:, 0]
            host_ptr = host[:, 136:144].copy().view(np.uint64)[:, 0]
            assert np.array_equal(dev_ptr != 0, host_ptr != 0)
            tris[:, 136:144] = host[:, 136:144]
            return (tris.tobytes(), download(sc.kd_tree.nodes, 20 * nn).tobytes(),
                    download(sc.kd_tree.triangle_indicies, 4 * ni).view(np.int32), lights, bounds)

    record, _, _ = rc.scene_record(_Uploaded())
    assert record == want


def test_trace_rays_equal_the_recorded_samples(workdir):
    """rt_trace_rays on the hazard ray set (on-split origins, NaN and infinite components, axis-parallel
    directions) against the Samples the reference's trace_ray recorded"""
    fx, run = gpu_case(workdir, rc.RAY_CASE)
    rays, want = fx["rays"], fx["samples"]
    col = reference.SAMPLE_FIELDS
    hit = want[:, col["hit"]][:, 0] == 1
    assert 0.2 < hit.mean() < 0.98
    bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)  # noqa: E731
    for mode in (rt.TRAVERSAL_BOUNDED, rt.TRAVERSAL_KD):
        hits, surf = rt.trace_rays(run.dev, rays, surface=True, traversal=mode)
        assert np.array_equal(hits["triangle"] >= 0, hit), (mode, np.nonzero((hits["triangle"] >= 0) != hit)[0][:8])
        tri = want[:, col["triangle"]][:, 0].astype(np.int64)
        bad = np.nonzero(hits["triangle"] != tri)[0]
        assert len(bad) == 0, (mode, "triangle", len(bad), bad[:8], hits["triangle"][bad[:8]], tri[bad[:8]])
        for field in ("position", "normal", "tangent", "albedo", "emittance"):
            a, b = bits(surf[field])[hit], bits(want[:, col[field]])[hit]
            bad = np.nonzero((a != b).any(axis=1))[0]
            assert len(bad) == 0, (mode, field, len(bad), bad[:8], surf[field][hit][bad[:3]],
                                   want[:, col[field]][hit][bad[:3]])


def test_tonemap_equals_the_recorded_bytes(workdir):
    """rt_tonemap of the cornell case's final frame against the bytes the reference's display pixel gives
    (draw_frame's and save_render's colour statement over the reference's correct_color)"""
    fx, run = gpu_case(workdir, rc.TONEMAP_CASE)
    got, g = render(fx, run, rt.KERNEL_WAVEFRONT, rt.TRAVERSAL_BOUNDED)
    helpers.assert_bitwise(got[-1], rc.fixture_frames(fx)[-1], what="cornell vs the recorded reference:")
    rgba = rt.tonemap(g)
    bad = np.nonzero((rgba != fx["tonemap_rgba"]).any(axis=1))[0]
    assert len(bad) == 0, (len(bad), bad[:8], rgba[bad[:3]], fx["tonemap_rgba"][bad[:3]])
    assert len(np.unique(rgba[:, :3])) > 50  # a real image, not one colour
