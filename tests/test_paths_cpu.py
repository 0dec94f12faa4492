"""The radiance query (rt_trace_paths, include/isaklm_rt.h) without a GPU:
the header, the binding and the argument checks, and the reference the GPU
tests (tests/test_gpu_paths.py) compare through — path_query_ref.
camera_samples, the mapping from a frame's camera samples to a ray list — is
pinned to the scalar code of independent_path.render and, with the scalar
trace_path, to the oracle's or_render, bit for bit.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import helpers
import independent_path as ip
import path_query_ref as pq
import rt

f32 = np.float32
E_INVALID = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")


def test_header_and_binding(tmp_path):
    text = open(os.path.join(INC, "isaklm_rt.h")).read()
    assert int(re.search(r"#define RT_ABI_VERSION (\d+)", text).group(1)) == 12
    assert rt.ABI_VERSION == 12 and rt.lib().rt_abi_version() == 12
    assert re.search(r"^#define RT_HAS_TRACE_PATHS 1$", text, re.M)
    m = re.search(r"int rt_trace_paths\(([^;]*)\);", text)
    assert m, "rt_trace_paths is not declared"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == ["rt_scene_t scene", "const float *rays_device", "uint32_t *rng_device", "long long n",
                      "float *radiance_device", "float *sq_luminance_device", "const RtPathOptions *opt"]
    assert re.search(r"void rt_default_path_options\(RtPathOptions \*opt\);", text)
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    fields = [name for name, _ in rt.RtPathOptions._fields_]
    assert fields == ["samples", "max_depth", "accumulate", "traversal", "stream", "stats_device"]
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "isaklm_rt.h"\n#ifndef RT_HAS_TRACE_PATHS\n'
                   '#error "no feature test"\n#endif\nint main(void) {\n  printf("%zu", sizeof(RtPathOptions));\n'
                   + "".join(f'  printf(" %zu", offsetof(RtPathOptions, {f}));\n' for f in fields)
                   + "  return 0;\n}\n")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", INC, str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [ctypes.sizeof(rt.RtPathOptions)] + [getattr(rt.RtPathOptions, f).offset for f in fields]
    L = rt.lib()
    vp = ctypes.c_void_p
    assert L.rt_trace_paths.argtypes == [vp, vp, vp, ctypes.c_longlong, vp, vp, ctypes.POINTER(rt.RtPathOptions)]
    assert L.rt_trace_paths.restype is ctypes.c_int
    assert L.rt_default_path_options.argtypes == [ctypes.POINTER(rt.RtPathOptions)]
    assert rt.PATH_STATS == ("rays", "paths", "trace_calls", "cut_paths", "max_depth")
    o = rt.path_options()
    assert (o.samples, o.max_depth, o.accumulate, o.traversal) == (1, 0, 0, rt.TRAVERSAL_BOUNDED)
    assert o.stream is None and o.stats_device is None


def test_argument_errors_without_a_device():
    """Every rejected call returns RT_E_INVALID before it looks at the scene or
    the device: the scene handle below is not a scene and the pointers are not
    device memory."""
    L = rt.lib()
    fake, good = 0x1000, 0x2000  # never dereferenced by a rejected call
    ok = dict(scene=fake, rays=good, rng=good, n=4, rad=good, sq=good)
    cases = [
        (dict(scene=None), "null scene"),
        (dict(rays=None), "null rays"),
        (dict(rng=None), "null rng"),
        (dict(rad=None), "null radiance"),
        (dict(rad=None, sq=None), "null radiance and sq"),
        (dict(n=-1), "n < 0"),
        (dict(n=1 << 31), "n > 2^31 - 1"),
        (dict(rays=good + 4), "rays not 8-B aligned"),
        (dict(rng=good + 2), "rng not 4-B aligned"),
        (dict(rad=good + 1), "radiance not 4-B aligned"),
        (dict(sq=good + 3), "sq not 4-B aligned"),
    ]
    for change, what in cases:
        a = dict(ok, **change)
        for opt in (ctypes.byref(rt.path_options()), None):  # (NULL: the default options)
            assert L.rt_trace_paths(a["scene"], a["rays"], a["rng"], a["n"], a["rad"], a["sq"], opt) == E_INVALID, what
            assert L.rt_last_error(), what
    for bad, what in ((dict(samples=-1), "samples < 0"), (dict(samples=(1 << 20) + 1), "samples > 2^20"),
                      (dict(max_depth=-1), "max_depth < 0"), (dict(max_depth=1 << 24), "max_depth > 2^24 - 1"),
                      (dict(accumulate=2), "accumulate 2"), (dict(accumulate=-1), "accumulate -1"),
                      (dict(traversal=77), "traversal"), (dict(stats=good + 4), "stats not 8-B aligned")):
        o = rt.path_options(**bad)
        assert L.rt_trace_paths(fake, good, good, 4, good, good, ctypes.byref(o)) == E_INVALID, what
        assert L.rt_trace_paths(fake, good, good, 0, good, good, ctypes.byref(o)) == E_INVALID, what + ", n = 0"
    # n == 0 with acceptable arguments: RT_OK, no launch, the scene is not looked at
    assert L.rt_trace_paths(fake, good, good, 0, good, None, None) == 0
    assert L.rt_trace_paths(fake, good, good, 0, good, good, ctypes.byref(rt.path_options(samples=0))) == 0
    rays, rng = np.zeros((4, 6), f32), np.zeros(4, np.uint32)
    for bad_call in (lambda: rt.trace_paths(None, np.zeros((4, 5), f32), rng),
                     lambda: rt.trace_paths(None, np.zeros(24, f32), rng),
                     lambda: rt.trace_paths(None, rays, np.zeros(3, np.uint32)),
                     lambda: rt.trace_paths(None, rays, np.zeros(4, np.int32)),
                     lambda: rt.trace_paths(None, rays, np.zeros(4, np.float32)),
                     lambda: rt.trace_paths(None, rays, rng, radiance=np.zeros((4, 3), np.float64)),
                     lambda: rt.trace_paths(None, rays, rng, radiance=np.zeros((3, 3), f32)),
                     lambda: rt.trace_paths(None, rays, rng, radiance=np.zeros((4, 3), f32), sq=np.zeros(5, f32)),
                     lambda: rt.trace_paths(None, rays, rng, sq=np.zeros(4, f32))):
        with pytest.raises(ValueError):
            bad_call()


# ---- the mapping from camera samples to rays ----
W = H = 8


class _Recorder:
    """stands in for independent_path.Scene in independent_path.render: records what trace_path is given"""

    def __init__(self):
        self.calls = []

    def trace_path(self, o, d, st):
        self.calls.append((o, d, st))
        return ip.v(0, 0, 0), st


@pytest.fixture(scope="module")
def cornell():
    path = helpers.scene_path("cornell")
    host = rt.HostScene(path)
    return path, host, np.asarray(host.camera.as_list(), f32)


def _cameras(cam):
    zero, wide = cam.copy(), cam.copy()
    zero[6] = 0.0
    wide[6] = 0.05
    return {"own": cam, "aperture 0": zero, "aperture 0.05": wide}


@pytest.mark.parametrize("which", ["own", "aperture 0", "aperture 0.05"])
def test_camera_samples_are_the_scalar_codes(cornell, which):
    """rays and post-draw RNG states of every pixel == what independent_path.render hands to trace_path"""
    cam = _cameras(cornell[2])[which]
    if which == "aperture 0.05":
        assert cam[6] > 0
    n = W * H
    seeds = ip.reference_seeds(n)
    rec = _Recorder()
    ip.render(rec, cam, W, H, 1, np.zeros((n, 3), f32), np.zeros(n, f32), np.zeros(n, np.int32), seeds.copy())
    assert len(rec.calls) == n
    want = np.array([list(o) + list(d) for o, d, _ in rec.calls], f32)
    want_st = np.array([st for _, _, st in rec.calls], np.uint32)
    rays, st = pq.camera_samples(cam, W, H, seeds)
    assert rays.dtype == f32 and rays.shape == (n, 6) and st.dtype == np.uint32
    assert np.array_equal(rays.view(np.uint32), want.view(np.uint32)), np.nonzero(rays != want)
    assert np.array_equal(st, want_st)
    if cam[6] == 0:  # every origin is the camera position
        assert np.array_equal(rays[:, :3], np.broadcast_to(cam[:3], (n, 3)))
    else:
        assert (rays[:, :3] != cam[:3]).any(axis=1).mean() > 0.9
    # a pixel subset: the same rays
    sub = np.array([5, 63, 0, 17])
    r2, s2 = pq.camera_samples(cam, W, H, seeds[sub], pixels=sub)
    assert np.array_equal(r2.view(np.uint32), rays[sub].view(np.uint32)) and np.array_equal(s2, st[sub])


def test_the_mapping_is_pinned_to_the_oracle(cornell):
    """scalar trace_path on camera_samples' output == one or_render pass from reset: fb, sq and rng, bitwise"""
    path, host, cam = cornell
    tri_bytes, _ = host.triangles_bytes()
    scene = ip.Scene(tri_bytes)
    n = W * H
    seeds = ip.reference_seeds(n)
    (fb, sq, cnt, rng), counters = helpers.oracle_render(path, W, H, 1, camera=cam)
    assert (cnt == 1).all() and counters["nee"] > 0 and (fb != 0).any()
    rays, st = pq.camera_samples(cam, W, H, seeds)
    pq.assert_same(pq.scalar_paths(scene, rays, st), (fb, sq, rng), "camera samples -> scalar trace_path vs or_render")
