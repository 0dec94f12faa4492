"""TEST INFRASTRUCTURE ONLY — ctypes wrapper of oracle/_ref/libref_rt.so: the
reference's own source, compiled as host C++ by oracle/Makefile.ref and driven
by oracle/ref_harness.cpp.  ReferenceScene mirrors oracle.OracleScene, so a
test can put the two side by side.

The library exists only where a copy of the reference does (oracle.build()
builds it there); elsewhere the recorded results in tests/golden/reference/
stand in for it.
"""
import ctypes
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "_ref", "libref_rt.so")
GLIBC_LIB_PATH = os.path.join(HERE, "_ref", "libref_rt_glibc.so")  # `make -f Makefile.ref glibc` (a measurement)
SAMPLE_FIELDS = {"hit": slice(0, 1), "triangle": slice(1, 2), "albedo": slice(2, 5), "emittance": slice(5, 8),
                 "roughness": slice(8, 9), "refractive_index": slice(9, 10), "extinction": slice(10, 11),
                 "transparent": slice(11, 12), "position": slice(12, 15), "normal": slice(15, 18),
                 "tangent": slice(18, 21), "bitangent": slice(21, 24)}  # columns of trace_rays' result

_libs = {}


def available():
    """the library is there, or can be built (oracle.build() does when the reference is present)"""
    return os.path.exists(LIB_PATH)


def lib(path=None):
    path = path or LIB_PATH
    if path not in _libs:
        L = ctypes.CDLL(path)
        vp, i, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
        L.ref_last_error.restype = ctypes.c_char_p
        L.ref_scene_load.argtypes = [ctypes.c_char_p, vp]
        L.ref_scene_load.restype = vp
        L.ref_scene_free.argtypes = [vp]
        L.ref_scene_free.restype = None
        L.ref_scene_counts.argtypes = [vp, ctypes.POINTER(i), ctypes.POINTER(i), ctypes.POINTER(i), ctypes.POINTER(i)]
        L.ref_scene_copy.argtypes = [vp, vp, vp, vp, vp, vp]
        L.ref_scene_copy.restype = None
        L.ref_seeds.argtypes = [i, i, vp]
        L.ref_seeds.restype = None
        L.ref_trace_rays.argtypes = [vp, vp, i, vp]
        L.ref_trace_rays.restype = None
        L.ref_scatter.argtypes = [vp, vp, vp, vp, i, vp, vp, vp, vp]
        L.ref_scatter.restype = None
        L.ref_direct_light.argtypes = [vp, vp, vp, vp, i, vp]
        L.ref_direct_light.restype = None
        L.ref_render.argtypes = [vp, vp, vp, vp, vp, vp, i, i, i, i, i, i, f]
        L.ref_correct_color.argtypes = [vp, i, vp]
        L.ref_correct_color.restype = None
        L.ref_tonemap.argtypes = [vp, vp, i, vp]
        L.ref_tonemap.restype = None
        _libs[path] = L
    return _libs[path]


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


def seeds(width, height, lib_path=None):
    """the seeds the reference's G_Buffer constructor draws for a width x height frame"""
    out = np.zeros(width * height, np.uint32)
    lib(lib_path).ref_seeds(width, height, _p(out))
    return out


class ReferenceScene:
    """The reference's Scene of one scene file (load_mesh, create_scene, create_kd_tree)."""

    def __init__(self, scene_path, lib_path=None):
        self.L = lib(lib_path)
        self.camera = np.zeros(7, np.float32)
        self.h = self.L.ref_scene_load(os.path.abspath(scene_path).encode(), _p(self.camera))
        if not self.h:
            raise RuntimeError("reference scene load failed: " + self.L.ref_last_error().decode())
        t, n, i, l = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        self.L.ref_scene_counts(self.h, ctypes.byref(t), ctypes.byref(n), ctypes.byref(i), ctypes.byref(l))
        self.ntris, self.nnodes, self.nindices, self.nlights = t.value, n.value, i.value, l.value

    def arrays(self):
        """(triangle bytes, node bytes, indices, lights, bounds) as oracle.OracleScene.arrays()"""
        tris = ctypes.create_string_buffer(self.ntris * 152)
        nodes = ctypes.create_string_buffer(max(self.nnodes, 1) * 20)
        idx = np.zeros(max(self.nindices, 1), np.int32)
        lights = np.zeros(max(self.nlights, 1), np.int32)
        bounds = np.zeros(6, np.float32)
        self.L.ref_scene_copy(self.h, ctypes.cast(tris, ctypes.c_void_p), ctypes.cast(nodes, ctypes.c_void_p),
                              _p(idx), _p(lights), _p(bounds))
        return (tris.raw, nodes.raw[: self.nnodes * 20], idx[: self.nindices], lights[: self.nlights], bounds)

    def trace_rays(self, rays):
        """trace_ray -> (n, 24) float32, columns SAMPLE_FIELDS (the whole Sample)"""
        rays = np.ascontiguousarray(rays, np.float32)
        out = np.zeros((len(rays), 24), np.float32)
        self.L.ref_trace_rays(self.h, _p(rays), len(rays), _p(out))
        return out

    def direct_light(self, pos, normal, rng):
        """sample_direct_light at n points -> (radiance (n, 3), rng after (n,))"""
        pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 3)
        normal = np.ascontiguousarray(normal, np.float32).reshape(-1, 3)
        state = np.array(rng, np.uint32).reshape(-1).copy()
        out = np.zeros((len(pos), 3), np.float32)
        self.L.ref_direct_light(self.h, _p(pos), _p(normal), _p(state), len(pos), _p(out))
        return out, state

    def render(self, camera, fb, sq, cnt, rng, width, height, passes, sample_count_arg=1, adaptive=True,
               min_samples=100, tolerance=0.05):
        """path_tracing() over `passes` passes on G_Buffer-layout arrays (modified in place)"""
        cam = np.ascontiguousarray(camera, np.float32)
        for a, dt in ((fb, np.float32), (sq, np.float32), (cnt, np.int32), (rng, np.uint32)):
            assert a.dtype == dt and a.flags["C_CONTIGUOUS"]
        assert fb.size == 3 * width * height and sq.size == cnt.size == rng.size == width * height
        if self.L.ref_render(self.h, _p(cam), _p(fb), _p(sq), _p(cnt), _p(rng), width, height, passes,
                             sample_count_arg, int(adaptive), min_samples, tolerance) != 0:
            raise RuntimeError("reference render failed: " + self.L.ref_last_error().decode())

    def __del__(self):
        try:
            if getattr(self, "h", None):
                self.L.ref_scene_free(self.h)
                self.h = None
        except Exception:
            pass


def scatter(ray_dir, sample22, inside, rng, lib_path=None):
    """get_scattered_light on n inputs laid out as or_scatter's ->
    (position, direction, weight, type, inside after, rng after)"""
    d = np.ascontiguousarray(ray_dir, np.float32)
    s = np.ascontiguousarray(sample22, np.float32)
    ins = np.ascontiguousarray(inside, np.int32)
    st = np.ascontiguousarray(rng, np.uint32)
    n = len(d)
    out = np.zeros((n, 9), np.float32)
    rng_out, in_out, ty_out = np.zeros(n, np.uint32), np.zeros(n, np.int32), np.zeros(n, np.int32)
    lib(lib_path).ref_scatter(_p(d), _p(s), _p(ins), _p(st), n, _p(out), _p(rng_out), _p(in_out), _p(ty_out))
    return out[:, 0:3], out[:, 3:6], out[:, 6:9], ty_out, in_out.astype(bool), rng_out


def correct_color(colors, lib_path=None):
    c = np.ascontiguousarray(colors, np.float32).reshape(-1, 3)
    out = np.zeros_like(c)
    lib(lib_path).ref_correct_color(_p(c), len(c), _p(out))
    return out


def tonemap(fb, cnt, lib_path=None):
    """the pixel of draw_frame / save_render -> (n, 4) uint8, rows as in the frame buffer"""
    fb = np.ascontiguousarray(fb, np.float32)
    cnt = np.ascontiguousarray(cnt, np.int32)
    out = np.zeros((len(cnt), 4), np.uint8)
    lib(lib_path).ref_tonemap(_p(fb), _p(cnt), len(cnt), _p(out))
    return out
