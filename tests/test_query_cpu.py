"""The ray-query API (rt_trace_rays / rt_camera_rays / rt_render_aov,
include/isaklm_rt.h ABI 10) without a GPU: argument errors are reported
before any device call, the record types have the header's sizes, and the
domain gate of csrc/query.hip stands on checked ground — inside
0.5 <= max|d_i| <= 2 the bounded traversal equals the plain KD traversal on
the host restatement (tests/native/bvh_trace_check.cpp, the device code's
float operations).  The kernel itself is compared with the oracle in
tests/test_gpu_query.py.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import helpers
import oracle
import rt

INC = os.path.join(helpers.ROOT, "include")
E_INVALID = -1


def test_record_sizes(tmp_path):
    assert rt.RAY_HIT.itemsize == 16 and rt.RAY_SURFACE.itemsize == 80
    assert rt.RAY_SURFACE.fields["t"][1] == 12 and rt.RAY_SURFACE.fields["normal"][1] == 16
    assert rt.RAY_SURFACE.fields["albedo"][1] == 48 and rt.RAY_SURFACE.fields["emittance"][1] == 64
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include "isaklm_rt.h"\n'
                   '_Static_assert(sizeof(RtRayHit) == 16, "hit");\n'
                   '_Static_assert(sizeof(RtRaySurface) == 80, "surface");\n'
                   '_Static_assert(offsetof(RtRaySurface, t) == 12 && offsetof(RtRaySurface, normal) == 16 && '
                   'offsetof(RtRaySurface, tangent) == 32 && offsetof(RtRaySurface, albedo) == 48 && '
                   'offsetof(RtRaySurface, emittance) == 64, "surface fields");\n'
                   f'_Static_assert(sizeof(RtQueryOptions) == {ctypes.sizeof(rt.RtQueryOptions)} && '
                   f'offsetof(RtQueryOptions, stream) == {rt.RtQueryOptions.stream.offset} && '
                   f'offsetof(RtQueryOptions, stats_device) == {rt.RtQueryOptions.stats_device.offset}, "options");\n'
                   f'_Static_assert(sizeof(RtAovBuffers) == {ctypes.sizeof(rt.RtAovBuffers)} && '
                   f'offsetof(RtAovBuffers, triangle) == {rt.RtAovBuffers.triangle.offset}, "aov");\n'
                   "int main(void){ return 0; }\n")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", INC, "-c", str(src), "-o", str(tmp_path / "s.o")],
                   check=True)


def test_default_query_options():
    o = rt.RtQueryOptions(7, 8, 9)
    rt.lib().rt_default_query_options(ctypes.byref(o))
    assert (o.traversal, o.stream, o.stats_device) == (rt.TRAVERSAL_BOUNDED, None, None)


def test_argument_errors_without_a_device():
    """Every rejected call returns RT_E_INVALID before it looks at the scene or
    the device: the scene handle below is not a scene and the pointers are not
    device memory."""
    L = rt.lib()
    fake_scene, good = 0x1000, 0x2000  # never dereferenced by a rejected call
    o = rt.query_options()
    cases = [
        (None, good, 4, good, None, "null scene"),
        (fake_scene, None, 4, good, None, "null rays"),
        (fake_scene, good, 4, None, None, "null hits"),
        (fake_scene, good, -1, good, None, "n < 0"),
        (fake_scene, good, 1 << 31, good, None, "n > 2^31 - 1"),
        (fake_scene, good + 4, 4, good, None, "rays not 8-B aligned"),
        (fake_scene, good, 4, good + 8, None, "hits not 16-B aligned"),
        (fake_scene, good, 4, good, good + 8, "surface not 16-B aligned"),
    ]
    for scene, rays, n, hits, surf, what in cases:
        assert L.rt_trace_rays(scene, rays, n, hits, surf, ctypes.byref(o)) == E_INVALID, what
        assert L.rt_last_error(), what
        assert L.rt_trace_rays(scene, rays, n, hits, surf, None) == E_INVALID, what  # (default options)
    cam = rt.Camera()
    assert L.rt_camera_rays(cam, 8, 8, None, None) == E_INVALID
    assert L.rt_camera_rays(cam, 8, 8, good + 4, None) == E_INVALID
    assert L.rt_camera_rays(cam, 0, 8, good, None) == E_INVALID
    assert L.rt_camera_rays(cam, 8, -1, good, None) == E_INVALID
    b = rt.RtAovBuffers(good, good, good, good)
    assert L.rt_render_aov(None, cam, 8, 8, ctypes.byref(b), None) == E_INVALID
    assert L.rt_render_aov(fake_scene, cam, 8, 8, None, None) == E_INVALID
    assert L.rt_render_aov(fake_scene, cam, 0, 8, ctypes.byref(b), None) == E_INVALID
    b = rt.RtAovBuffers(good + 2, good, good, good)
    assert L.rt_render_aov(fake_scene, cam, 8, 8, ctypes.byref(b), None) == E_INVALID


# ---- the gate's domain on the host restatement ----
@pytest.fixture(scope="module")
def trace_check(tmp_path_factory):
    return helpers.build_native(tmp_path_factory.mktemp("query"), "bvh_trace_check")


def _rescaled(g, unit, target):
    """unit directions rescaled so that max|d_i| is exactly `target` (an array or a scalar): the largest
    component is set to +-target itself, the others scaled by target / max (rounded)"""
    a = np.abs(unit)
    k = a.argmax(axis=1)
    m = a[np.arange(len(a)), k]
    t = np.broadcast_to(np.asarray(target, np.float32), m.shape)
    d = (unit * (t / m)[:, None]).astype(np.float32)
    d[np.arange(len(d)), k] = np.copysign(t, unit[np.arange(len(a)), k])
    return d


@pytest.mark.parametrize("name", ["cornell", "room_small"])
def test_bounded_equals_kd_inside_the_gate(trace_check, tmp_path, name):
    """8,192 seeded rays per set from inside the scene box, max|d_i| exactly
    0.5 (the gate's lower edge), exactly 2.0 (its upper edge) and seeded values
    between: bounded == plain KD on every ray."""
    path = helpers.scene_path(name)
    bounds = oracle.OracleScene(path).arrays()[4]
    g = np.random.default_rng(2024)
    N = 8192
    sets = []
    for target in (np.float32(0.5), np.float32(2.0), None):
        o = g.uniform(bounds[:3], bounds[3:], (N, 3)).astype(np.float32)
        u = g.normal(size=(N, 3))
        u = (u / np.linalg.norm(u, axis=1)[:, None]).astype(np.float32)
        t = target if target is not None else g.uniform(0.5, 2.0, N).astype(np.float32)
        d = _rescaled(g, u, t)
        assert np.array_equal(np.abs(d).max(axis=1), np.broadcast_to(t, (N,)))
        sets.append(np.concatenate([o, d], axis=1))
    rays = np.concatenate(sets).astype(np.float32)
    f = str(tmp_path / "rays.f32")
    rays.tofile(f)
    r = subprocess.run([trace_check, path, "file", f], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, OMP_NUM_THREADS="4"))
    assert r.returncode == 0 and f"rays {3 * N} mismatches 0;" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
