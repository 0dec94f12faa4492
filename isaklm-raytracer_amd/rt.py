"""ctypes binding of include/isaklm_rt.h — the host-side mirror of the
reference's render interface (create_scene / G_Buffer / Camera / render /
save_render, rt/main.cu:97-132) used by the tests, smoke() and bench.py.

The product path is the in-tree libisaklm_rt.so (HIP kernels for gfx950);
importing this module fails loudly if it is missing — there is no CPU
fallback.
"""
import contextlib
import ctypes
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libisaklm_rt.so")
# tooling only (tools/ab.py A/B of kernel builds): load another build of the same library
LIB_PATH = os.environ.get("ISAKLM_RT_LIB_OVERRIDE", LIB_PATH)


class Vec3D(ctypes.Structure):
    _fields_ = [("x", ctypes.c_float), ("y", ctypes.c_float), ("z", ctypes.c_float)]


class Bounding_Box(ctypes.Structure):
    _fields_ = [("min", Vec3D), ("max", Vec3D)]


class KD_Tree(ctypes.Structure):
    _fields_ = [("bounding_box", Bounding_Box), ("nodes", ctypes.c_void_p), ("triangle_indicies", ctypes.c_void_p)]


class Scene(ctypes.Structure):  # rt/scene.cuh:114-121
    _fields_ = [("triangles", ctypes.c_void_p), ("triangle_count", ctypes.c_int),
                ("light_indicies", ctypes.c_void_p), ("light_count", ctypes.c_int), ("kd_tree", KD_Tree)]


class G_Buffer(ctypes.Structure):  # rt/screen.cuh:15-21
    _fields_ = [("frame_buffer", ctypes.c_void_p), ("squared_luminance", ctypes.c_void_p),
                ("sample_count", ctypes.c_void_p), ("random_numbers", ctypes.c_void_p)]


class Camera(ctypes.Structure):  # rt/camera.cuh:15-26
    _fields_ = [("position", Vec3D), ("yaw", ctypes.c_float), ("pitch", ctypes.c_float),
                ("FOV", ctypes.c_float), ("aperture_radius", ctypes.c_float)]

    def as_list(self):
        p = self.position
        return [p.x, p.y, p.z, self.yaw, self.pitch, self.FOV, self.aperture_radius]


class RtOptions(ctypes.Structure):
    _fields_ = [("width", ctypes.c_int), ("height", ctypes.c_int), ("passes", ctypes.c_int),
                ("adaptive", ctypes.c_int), ("min_samples", ctypes.c_int), ("tolerance", ctypes.c_float),
                ("max_depth", ctypes.c_int), ("kernel", ctypes.c_int), ("stream", ctypes.c_void_p),
                ("counters_device", ctypes.c_void_p), ("wave_times_device", ctypes.c_void_p),
                ("wf_tail", ctypes.c_int), ("wf_finish_waves", ctypes.c_int), ("profile", ctypes.c_int),
                ("wf_descent_cap", ctypes.c_int), ("wf_postpone", ctypes.c_int), ("wf_wide", ctypes.c_int),
                ("shard_id", ctypes.c_int), ("num_shards", ctypes.c_int), ("wf_pipelines", ctypes.c_int),
                ("wf_long_depth", ctypes.c_int), ("traversal", ctypes.c_int), ("overlap", ctypes.c_int),
                ("check_interval", ctypes.c_int), ("debug", ctypes.c_int), ("coalesce_passes", ctypes.c_int)]


class RtProfile(ctypes.Structure):
    _fields_ = [("iterations", ctypes.c_int), ("trace_launches", ctypes.c_int), ("shade_launches", ctypes.c_int),
                ("finish_launches", ctypes.c_int), ("start_ms", ctypes.c_float), ("trace_ms", ctypes.c_float),
                ("shade_ms", ctypes.c_float), ("finish_ms", ctypes.c_float), ("call_ms", ctypes.c_float),
                ("trace_union_ms", ctypes.c_float), ("pipelines", ctypes.c_int)]


class RtQueryOptions(ctypes.Structure):
    _fields_ = [("traversal", ctypes.c_int), ("stream", ctypes.c_void_p), ("stats_device", ctypes.c_void_p)]


class RtPathOptions(ctypes.Structure):
    _fields_ = [("samples", ctypes.c_int), ("max_depth", ctypes.c_int), ("accumulate", ctypes.c_int),
                ("traversal", ctypes.c_int), ("stream", ctypes.c_void_p), ("stats_device", ctypes.c_void_p)]


class RtSampler(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_int), ("width", ctypes.c_int), ("height", ctypes.c_int), ("camera", Camera),
                ("ortho_half_width", ctypes.c_float), ("pixels_device", ctypes.c_void_p),
                ("points_device", ctypes.c_void_p)]


class RtAdaptive(ctypes.Structure):
    _fields_ = [("min_samples", ctypes.c_int), ("tolerance", ctypes.c_float)]


class RtAovBuffers(ctypes.Structure):
    _fields_ = [("depth", ctypes.c_void_p), ("normal", ctypes.c_void_p), ("albedo", ctypes.c_void_p),
                ("triangle", ctypes.c_void_p)]


class RtDenoiseOptions(ctypes.Structure):
    _fields_ = [("iterations", ctypes.c_int), ("sigma_lum", ctypes.c_float), ("sigma_depth", ctypes.c_float),
                ("normal_log2", ctypes.c_int), ("demodulate", ctypes.c_int), ("stream", ctypes.c_void_p)]


class RtReprojectOptions(ctypes.Structure):
    _fields_ = [("max_history", ctypes.c_int), ("depth_tol", ctypes.c_float), ("normal_min", ctypes.c_float),
                ("match_triangle", ctypes.c_int), ("stream", ctypes.c_void_p), ("stats_device", ctypes.c_void_p)]


# RtRayHit (16 B) and RtRaySurface (80 B) as numpy record types
RAY_HIT = np.dtype([("triangle", np.int32), ("bx", np.float32), ("by", np.float32), ("bz", np.float32)])
RAY_SURFACE = np.dtype([("position", np.float32, 3), ("t", np.float32), ("normal", np.float32, 3),
                        ("_pad0", np.float32), ("tangent", np.float32, 3), ("_pad1", np.float32),
                        ("albedo", np.float32, 3), ("_pad2", np.float32), ("emittance", np.float32, 3),
                        ("_pad3", np.float32)])
QUERY_STATS = ("rays", "hits", "kd_rays")  # RtQueryOptions.stats_device [0..2]


def last_profile():
    """Kernel timing of the last rt_render with options(profile=True) on this device."""
    p = RtProfile()
    check(lib().rt_last_profile(ctypes.byref(p)))
    return {k: getattr(p, k) for k, _ in RtProfile._fields_}


def profile_history(reset=False):
    """RtProfile of every profiled rt_render since the last reset, oldest first
    (rt_profile_history: waits for those calls' kernels, not for the chain)."""
    n = ctypes.c_int(0)
    check(lib().rt_profile_history(None, 0, ctypes.byref(n), 0))
    buf = (RtProfile * max(n.value, 1))()
    check(lib().rt_profile_history(buf, n.value, ctypes.byref(n), int(reset)))
    return [{k: getattr(buf[i], k) for k, _ in RtProfile._fields_} for i in range(n.value)]


DEV_HIST_BINS = 18


class RtDeviations(ctypes.Structure):
    _fields_ = [("watchdog_paths", ctypes.c_ulonglong), ("cut_paths", ctypes.c_ulonglong),
                ("max_deep_depth", ctypes.c_ulonglong), ("deep_paths", ctypes.c_ulonglong),
                ("deep_hist", ctypes.c_ulonglong * DEV_HIST_BINS),
                ("bounded_checked", ctypes.c_ulonglong), ("bounded_mismatches", ctypes.c_ulonglong),
                ("mismatch_ray", ctypes.c_float * 6),
                ("owed_pixels", ctypes.c_ulonglong), ("owed_passes", ctypes.c_ulonglong),
                ("long_safety_quits", ctypes.c_ulonglong), ("stranded_pixels", ctypes.c_ulonglong),
                ("check_dropped", ctypes.c_ulonglong), ("linger_expiries", ctypes.c_ulonglong),
                ("long_closed", ctypes.c_ulonglong), ("wide_overflows", ctypes.c_ulonglong)]


HANDOFF_FIELDS = ("owed_pixels", "owed_passes", "long_safety_quits", "stranded_pixels", "check_dropped",
                  "linger_expiries", "long_closed", "wide_overflows")


def deviation_stats(reset=False):
    """Always-on deviation statistics of every rt_render on this device since
    the last reset (rt_deviation_stats): watchdog / depth-limit cuts, the
    histogram of paths that ended at depth >= 64 (bin k: [64*2^k, 64*2^(k+1))),
    the guard's checks, and the deep-path hand-off's events (owed passes of
    chained calls; safety-net exits, stranded pixels, dropped guard records
    and linger expiries, which a working render keeps at 0)."""
    d = RtDeviations()
    check(lib().rt_deviation_stats(ctypes.byref(d), int(reset)))
    out = {"watchdog_paths": d.watchdog_paths, "cut_paths": d.cut_paths, "max_deep_depth": d.max_deep_depth,
           "deep_paths": d.deep_paths, "deep_hist": [int(v) for v in d.deep_hist],
           "bounded_checked": int(d.bounded_checked), "bounded_mismatches": int(d.bounded_mismatches),
           "mismatch_ray": [float(v) for v in d.mismatch_ray]}
    out.update({k: int(getattr(d, k)) for k in HANDOFF_FIELDS})
    return out


def kd_cert_stats(reset=False):
    """rt_kd_cert_stats: (certified, fallback) hit rays of the bounded traversal
    in counting renders (TRAVERSAL_BOUNDED_COUNTED) since the last reset."""
    if not hasattr(lib(), "rt_kd_cert_stats"):
        raise RtError(f"{LIB_PATH} was built before rt_kd_cert_stats was added (within ABI {ABI_VERSION}): rebuild it")
    a, b = ctypes.c_ulonglong(0), ctypes.c_ulonglong(0)
    check(lib().rt_kd_cert_stats(ctypes.byref(a), ctypes.byref(b), int(reset)))
    return int(a.value), int(b.value)


def join(stream=None):
    """rt_join: `stream` (None: the host) waits for every render's device work,
    chained calls' deep-path tails included."""
    check(lib().rt_join(stream))


ABI_VERSION = 12  # RT_ABI_VERSION of include/isaklm_rt.h
E_INCOMPLETE = -7  # RT_E_INCOMPLETE: a join found stranded pixels
DEBUG_CALL_LOG, DEBUG_LONG_LOG, DEBUG_CHECK_FAULT, DEBUG_LONG_QUIT = 1, 2, 4, 8  # RtOptions.debug bits
DEBUG_SERIAL_LONG_FIRST, DEBUG_SERIAL_FIN_FIRST = 16, 32  # (tests: serialised dispatch in either order)
DEBUG_COUNT_LONG_ONLY = 128  # (measurement: a counted call in which only wf_long counts, tools/wide_rounds.py)
DEBUG_WIDE_CAP1 = 64  # (tests: wf_long's wave-wide s_min query overflows at once; deviation_stats wide_overflows)
DEBUG_BUDGET1 = 256  # (tests: a counted call's finisher parks its s_min queries after one body of the wave's work)
TRIANGLE_BYTES = 152
NODE_BYTES = 20
COUNTER_NAMES = ["node", "tri", "hit", "texel", "nee", "sample", "skip", "ray", "watchdog", "maxdepth"]
FINISH_COUNTER_NAMES = ["finish_node", "finish_tri", "finish_ray", "cand", "plane", "deep_push", "t_descend", "t_leaves",
                        "t_fetch", "rounds", "chunks", "bary", "wide_calls", "wide_rounds", "t_wide", "t_wide_load", "t_wide_leaf", "t_wide_expand",
                       "t_leaf_wait", "t_leaf_setup", "t_leaf_test", "t_leaf_bary", "spill_push", "spill_pop",
                        "pend_lanes", "leaf_tests", "t_desc_wait", "b_bvh_node", "b_bvh_tri", "b_bary"]
N_COUNTERS = 40

_lib = None


class RtError(RuntimeError):
    pass


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RtError(f"{LIB_PATH} is missing: run __graft_entry__.build() (no CPU fallback exists)")
        L = ctypes.CDLL(LIB_PATH)
        vp, i, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
        L.rt_last_error.restype = ctypes.c_char_p
        L.rt_version.restype = ctypes.c_char_p
        L.rt_device_alloc.argtypes = [ctypes.POINTER(vp), sz]
        L.rt_free.argtypes = [vp]
        L.rt_upload.argtypes = [vp, vp, sz]
        L.rt_download.argtypes = [vp, vp, sz]
        L.rt_memset.argtypes = [vp, i, sz]
        L.rt_device_count.argtypes = [ctypes.POINTER(i)]
        L.rt_set_device.argtypes = [i]
        L.rt_host_free.argtypes = [vp]
        L.rt_host_free.restype = None
        L.rt_gbuffer_save.argtypes = [G_Buffer, i, i, i, ctypes.c_char_p]
        L.rt_gbuffer_load.argtypes = [ctypes.c_char_p, G_Buffer, i, i, ctypes.POINTER(i)]
        L.rt_decode_image.argtypes = [ctypes.c_char_p, ctypes.POINTER(vp), ctypes.POINTER(i), ctypes.POINTER(i)]
        L.rt_decode_image_memory.argtypes = [vp, sz, ctypes.POINTER(vp), ctypes.POINTER(i), ctypes.POINTER(i)]
        L.rt_gbuffer_seeds.argtypes = [vp, sz, ctypes.c_uint64]
        L.rt_gbuffer_create.argtypes = [i, i, ctypes.c_uint64, ctypes.POINTER(G_Buffer)]
        L.rt_gbuffer_destroy.argtypes = [ctypes.POINTER(G_Buffer)]
        L.rt_host_scene_create.argtypes = [ctypes.POINTER(vp)]
        L.rt_host_scene_destroy.argtypes = [vp]
        L.rt_host_scene_destroy.restype = None
        L.rt_host_scene_load_mesh.argtypes = [vp, ctypes.c_char_p, ctypes.c_char_p, vp, vp, i]
        L.rt_host_scene_load_file.argtypes = [vp, ctypes.c_char_p, ctypes.POINTER(Camera)]
        L.rt_host_scene_triangles.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(i)]
        L.rt_generate_scene.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, sz]
        L.rt_build_kd_tree.argtypes = [vp, i, ctypes.POINTER(vp), ctypes.POINTER(i), ctypes.POINTER(vp),
                                       ctypes.POINTER(i), ctypes.POINTER(Bounding_Box)]
        L.rt_create_scene.argtypes = [vp, ctypes.POINTER(Scene), ctypes.POINTER(i), ctypes.POINTER(i)]
        L.rt_destroy_scene.argtypes = [ctypes.POINTER(Scene)]
        L.rt_scene_prepare.argtypes = [ctypes.POINTER(Scene), ctypes.POINTER(vp)]
        L.rt_scene_prepare_counts.argtypes = [ctypes.POINTER(Scene), i, i, ctypes.POINTER(vp)]
        L.rt_scene_prepare_host.argtypes = [vp, i, vp, i, vp, i, vp, i, Bounding_Box, ctypes.POINTER(vp)]
        L.rt_scene_release.argtypes = [vp]
        L.rt_scene_info.argtypes = [vp, ctypes.POINTER(sz), ctypes.POINTER(i), ctypes.POINTER(i),
                                    ctypes.POINTER(i), ctypes.POINTER(i)]
        L.rt_default_options.argtypes = [ctypes.POINTER(RtOptions)]
        L.rt_default_options.restype = None
        L.rt_render.argtypes = [vp, G_Buffer, Camera, i, ctypes.POINTER(RtOptions)]
        L.rt_tonemap.argtypes = [G_Buffer, vp, i, i, vp]
        L.rt_save_render.argtypes = [G_Buffer, i, i, ctypes.c_char_p]
        L.rt_deviation_stats.argtypes = [ctypes.POINTER(RtDeviations), i]
        if hasattr(L, "rt_kd_cert_stats"):  # (added within ABI 12: an earlier ABI-12 library lacks it)
            L.rt_kd_cert_stats.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), ctypes.POINTER(ctypes.c_ulonglong), i]
        L.rt_join.argtypes = [vp]
        L.rt_profile_history.argtypes = [ctypes.POINTER(RtProfile), i, ctypes.POINTER(i), i]
        L.rt_default_query_options.argtypes = [ctypes.POINTER(RtQueryOptions)]
        L.rt_default_query_options.restype = None
        L.rt_trace_rays.argtypes = [vp, vp, ctypes.c_longlong, vp, vp, ctypes.POINTER(RtQueryOptions)]
        L.rt_occluded.argtypes = [vp, vp, vp, ctypes.c_longlong, vp, ctypes.POINTER(RtQueryOptions)]
        L.rt_default_path_options.argtypes = [ctypes.POINTER(RtPathOptions)]
        L.rt_default_path_options.restype = None
        L.rt_trace_paths.argtypes = [vp, vp, vp, ctypes.c_longlong, vp, vp, ctypes.POINTER(RtPathOptions)]
        L.rt_camera_rays.argtypes = [Camera, i, i, vp, vp]
        if hasattr(L, "rt_sample_paths"):  # (added within ABI 12: an earlier ABI-12 library lacks it)
            L.rt_sample_paths.argtypes = [vp, ctypes.POINTER(RtSampler), vp, ctypes.c_longlong, vp, vp, vp,
                                          ctypes.POINTER(RtPathOptions)]
            L.rt_sampler_rays.argtypes = [ctypes.POINTER(RtSampler), vp, ctypes.c_longlong, vp, vp]
            L.rt_sampler_rays_host.argtypes = [ctypes.POINTER(RtSampler), vp, ctypes.c_longlong, vp]
        if hasattr(L, "rt_sample_paths_adaptive"):  # (added within ABI 12: an earlier ABI-12 library lacks it)
            L.rt_sample_paths_adaptive.argtypes = [vp, ctypes.POINTER(RtSampler), vp, ctypes.c_longlong, vp, vp, vp,
                                                   ctypes.POINTER(RtPathOptions), ctypes.POINTER(RtAdaptive)]
        if hasattr(L, "rt_convergence"):  # (added within ABI 12: an earlier ABI-12 library lacks it)
            L.rt_convergence.argtypes = [vp, vp, vp, ctypes.c_longlong, i, ctypes.c_float, vp, vp, vp]
            L.rt_convergence_host.argtypes = [vp, vp, vp, ctypes.c_longlong, i, ctypes.c_float, vp, vp]
        L.rt_render_aov.argtypes = [vp, Camera, i, i, ctypes.POINTER(RtAovBuffers), ctypes.POINTER(RtQueryOptions)]
        L.rt_default_denoise_options.argtypes = [ctypes.POINTER(RtDenoiseOptions)]
        L.rt_default_denoise_options.restype = None
        L.rt_denoise.argtypes = [G_Buffer, ctypes.POINTER(RtAovBuffers), i, i, vp, ctypes.POINTER(RtDenoiseOptions)]
        L.rt_denoise_host.argtypes = [vp, vp, vp, vp, vp, vp, i, i, vp, ctypes.POINTER(RtDenoiseOptions)]
        L.rt_tonemap_rgb.argtypes = [vp, vp, i, i, vp]
        if hasattr(L, "rt_reproject"):  # (added within ABI 12: an earlier ABI-12 library lacks it)
            L.rt_default_reproject_options.argtypes = [ctypes.POINTER(RtReprojectOptions)]
            L.rt_default_reproject_options.restype = None
            L.rt_reproject.argtypes = [G_Buffer, ctypes.POINTER(RtAovBuffers), Camera, ctypes.POINTER(RtAovBuffers),
                                       Camera, i, i, G_Buffer, ctypes.POINTER(RtReprojectOptions)]
            L.rt_reproject_host.argtypes = [vp, vp, vp, vp, vp, vp, Camera, vp, vp, vp, Camera, i, i, vp, vp, vp, vp,
                                            ctypes.POINTER(RtReprojectOptions)]
        if hasattr(L, "rt_sample_aov"):  # (added within ABI 12: an earlier ABI-12 library lacks it)
            smp = ctypes.POINTER(RtSampler)
            L.rt_sample_aov.argtypes = [vp, smp, ctypes.c_longlong, ctypes.POINTER(RtAovBuffers),
                                        ctypes.POINTER(RtQueryOptions)]
            L.rt_denoise_sampler.argtypes = [G_Buffer, ctypes.POINTER(RtAovBuffers), smp, vp,
                                             ctypes.POINTER(RtDenoiseOptions)]
            L.rt_denoise_sampler_host.argtypes = [vp, vp, vp, vp, vp, vp, smp, vp, ctypes.POINTER(RtDenoiseOptions)]
            L.rt_reproject_sampler.argtypes = [G_Buffer, ctypes.POINTER(RtAovBuffers), smp, ctypes.POINTER(RtAovBuffers),
                                               smp, G_Buffer, ctypes.POINTER(RtReprojectOptions)]
            L.rt_reproject_sampler_host.argtypes = [vp, vp, vp, vp, vp, vp, smp, vp, vp, vp, smp, vp, vp, vp, vp,
                                                    ctypes.POINTER(RtReprojectOptions)]
        L.rt_shutdown.restype = None
        L.rt_abi_version.restype = i
        if L.rt_abi_version() != ABI_VERSION:
            raise RtError(f"{LIB_PATH}: ABI version {L.rt_abi_version()}, this binding expects {ABI_VERSION} "
                          "(rebuild with __graft_entry__.build())")
        _lib = L
    return _lib


def check(rc):
    if rc != 0:
        raise RtError(f"rt error {rc}: {lib().rt_last_error().decode()}")


def _ptr(a):
    return ctypes.c_void_p(a.ctypes.data)


def generate_scene(name, out_dir):
    buf = ctypes.create_string_buffer(4096)
    check(lib().rt_generate_scene(name.encode(), out_dir.encode(), buf, 4096))
    return buf.value.decode()


def seeds(count, skip=0):
    out = np.zeros(count, dtype=np.uint32)
    check(lib().rt_gbuffer_seeds(_ptr(out), count, skip))
    return out


class HostScene:
    """Host triangle list (create_models / load_mesh, rt/create_models.cuh:17)."""

    def __init__(self, scene_path=None):
        h = ctypes.c_void_p()
        check(lib().rt_host_scene_create(ctypes.byref(h)))
        self.h = h
        self.camera = Camera()
        if scene_path:
            check(lib().rt_host_scene_load_file(self.h, scene_path.encode(), ctypes.byref(self.camera)))

    def load_mesh(self, obj, mat, offset, matrix, smooth=False):
        off = np.asarray(offset, dtype=np.float32)
        m = np.asarray(matrix, dtype=np.float32).reshape(9)
        check(lib().rt_host_scene_load_mesh(self.h, obj.encode(), mat.encode(), _ptr(off), _ptr(m), int(smooth)))

    def triangles_bytes(self):
        p, n = ctypes.c_void_p(), ctypes.c_int()
        check(lib().rt_host_scene_triangles(self.h, ctypes.byref(p), ctypes.byref(n)))
        return ctypes.string_at(p, n.value * TRIANGLE_BYTES), n.value

    def triangle_ptr(self):
        p, n = ctypes.c_void_p(), ctypes.c_int()
        check(lib().rt_host_scene_triangles(self.h, ctypes.byref(p), ctypes.byref(n)))
        return p, n.value

    def __del__(self):
        try:
            if getattr(self, "h", None):
                lib().rt_host_scene_destroy(self.h)
                self.h = None
        except Exception:
            pass


def decode_image(path=None, data=None):
    """stbi_load(path, &w, &h, &n, 4) as make_texture calls it (rt/scene.cuh:33):
    RGBA8 (H, W, 4) uint8, rows in file order.  PNG and baseline JPEG."""
    p, w, h = ctypes.c_void_p(), ctypes.c_int(), ctypes.c_int()
    if data is not None:
        buf = np.frombuffer(bytes(data), dtype=np.uint8)
        check(lib().rt_decode_image_memory(_ptr(buf), buf.nbytes, ctypes.byref(p), ctypes.byref(w), ctypes.byref(h)))
    else:
        check(lib().rt_decode_image(path.encode(), ctypes.byref(p), ctypes.byref(w), ctypes.byref(h)))
    try:
        n = w.value * h.value * 4
        return np.frombuffer(ctypes.string_at(p, n), dtype=np.uint8).reshape(h.value, w.value, 4).copy()
    finally:
        lib().rt_host_free(p)


def build_kd_tree(tri_ptr, n):
    """create_kd_tree on the host -> (nodes bytes, indices int32 array, bounds[6])."""
    L = lib()
    nodes, idx = ctypes.c_void_p(), ctypes.c_void_p()
    nn, ni = ctypes.c_int(), ctypes.c_int()
    bb = Bounding_Box()
    check(L.rt_build_kd_tree(tri_ptr, n, ctypes.byref(nodes), ctypes.byref(nn), ctypes.byref(idx),
                             ctypes.byref(ni), ctypes.byref(bb)))
    nb = ctypes.string_at(nodes, nn.value * NODE_BYTES)
    ib = np.frombuffer(ctypes.string_at(idx, ni.value * 4), dtype=np.int32).copy()
    L.rt_host_free(nodes)
    L.rt_host_free(idx)
    return nb, ib, [bb.min.x, bb.min.y, bb.min.z, bb.max.x, bb.max.y, bb.max.z]


class DeviceScene:
    """create_scene (rt/create_scene.cuh:18) -> reference-layout device Scene,
    then rt_scene_prepare -> traversal layout.  rt_scene_prepare takes the
    Scene alone (the reference's Scene has no node/index counts); the counts
    rt_create_scene reports are kept only to cross-check what prepare derived."""

    def __init__(self, host_scene):
        self.scene = Scene()
        nn, ni = ctypes.c_int(), ctypes.c_int()
        check(lib().rt_create_scene(host_scene.h, ctypes.byref(self.scene), ctypes.byref(nn), ctypes.byref(ni)))
        self.node_count, self.index_count = nn.value, ni.value
        self.prepared = ctypes.c_void_p()
        check(lib().rt_scene_prepare(ctypes.byref(self.scene), ctypes.byref(self.prepared)))

    def info(self):
        b, t, n, i, d = ctypes.c_size_t(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        check(lib().rt_scene_info(self.prepared, ctypes.byref(b), ctypes.byref(t), ctypes.byref(n), ctypes.byref(i),
                                  ctypes.byref(d)))
        return {"device_bytes": b.value, "triangles": t.value, "nodes": n.value, "indices": i.value,
                "max_depth": d.value, "lights": self.scene.light_count}

    def release(self):
        if getattr(self, "prepared", None):
            lib().rt_scene_release(self.prepared)
            self.prepared = None
        if getattr(self, "scene", None) is not None and self.scene.triangles:
            lib().rt_destroy_scene(ctypes.byref(self.scene))

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass


class GBuffer:
    """G_Buffer (rt/screen.cuh:22-46) on the device; seeds = mt19937 outputs
    [seed_skip, seed_skip + W*H)."""

    def __init__(self, width, height, seed_skip=0):
        self.width, self.height = width, height
        self.g = G_Buffer()
        check(lib().rt_gbuffer_create(width, height, seed_skip, ctypes.byref(self.g)))

    @property
    def n(self):
        return self.width * self.height

    ARRAYS = {"frame_buffer": (np.float32, (3,)), "squared_luminance": (np.float32, ()),
              "sample_count": (np.int32, ()), "random_numbers": (np.uint32, ())}

    def array(self, name):
        """one of the G_Buffer's four arrays (ARRAYS) as a DeviceArray that does not own it"""
        dtype, per = self.ARRAYS[name]
        return DeviceArray.at(getattr(self.g, name), (self.n,) + per, dtype)

    def download(self):
        """(fb (n, 3) float32, sq (n,) float32, cnt (n,) int32, rng (n,) uint32)"""
        return tuple(self.array(name).read() for name in self.ARRAYS)

    def upload(self, fb, sq, cnt, rng):
        for name, a in zip(self.ARRAYS, (fb, sq, cnt, rng)):
            self.array(name).upload(a)

    def save(self, path, sample_count):
        """checkpoint (rt_gbuffer_save): the whole progressive state + the caller's sample count"""
        check(lib().rt_gbuffer_save(self.g, self.width, self.height, sample_count, str(path).encode()))

    def load(self, path):
        """resume (rt_gbuffer_load); returns the saved sample count"""
        sc = ctypes.c_int()
        check(lib().rt_gbuffer_load(str(path).encode(), self.g, self.width, self.height, ctypes.byref(sc)))
        return sc.value

    def free(self):
        if getattr(self, "g", None) is not None and self.g.frame_buffer:
            lib().rt_gbuffer_destroy(ctypes.byref(self.g))

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


KERNEL_MEGA = 0
KERNEL_WAVEFRONT = 1
TRAVERSAL_BOUNDED = 0
TRAVERSAL_KD = 1
TRAVERSAL_BOUNDED_COUNTED = 2  # measurement: the bounded queue trace kernel counts its own work


def options(width, height, passes=1, adaptive=True, min_samples=100, tolerance=0.05, max_depth=0, stream=None,
            counters=None, kernel=KERNEL_MEGA, wf_tail=0, wf_finish_waves=0, profile=False, wf_descent_cap=0,
            wf_postpone=0, wf_wide=0, shard_id=0, num_shards=1, wave_times=None, wf_pipelines=0, wf_long_depth=0,
            traversal=None, overlap=False, check_interval=0, debug=0, coalesce_passes=0):
    """RtOptions; traversal: TRAVERSAL_BOUNDED / TRAVERSAL_KD (None: the
    library default, or RT_TRAVERSAL from the environment); overlap: chained
    calls (RtOptions.overlap: join before reading the frame); check_interval:
    the bounded traversal's run-time guard (0: the library default, 1 ray in
    4096; < 0: off); coalesce_passes: chained calls of fewer passes are
    coalesced up to this many (0: the library default 256; < 0: off)."""
    o = RtOptions()
    lib().rt_default_options(ctypes.byref(o))
    o.width, o.height, o.passes = width, height, passes
    o.adaptive, o.min_samples, o.tolerance, o.max_depth = int(adaptive), min_samples, tolerance, max_depth
    o.kernel = kernel
    o.stream = stream
    o.counters_device = counters
    o.wf_tail, o.wf_finish_waves, o.profile = wf_tail, wf_finish_waves, int(profile)
    o.wf_descent_cap, o.wf_postpone, o.wf_wide = wf_descent_cap, wf_postpone, wf_wide
    o.shard_id, o.num_shards = shard_id, num_shards
    o.wave_times_device = wave_times
    o.wf_pipelines = wf_pipelines
    o.wf_long_depth = wf_long_depth
    o.overlap, o.check_interval, o.debug = int(overlap), check_interval, debug
    o.coalesce_passes = coalesce_passes
    if traversal is None and os.environ.get("RT_TRAVERSAL"):
        traversal = {"bounded": TRAVERSAL_BOUNDED, "kd": TRAVERSAL_KD,
                     "bounded_counted": TRAVERSAL_BOUNDED_COUNTED}[os.environ["RT_TRAVERSAL"]]
    if traversal is not None:
        o.traversal = traversal
    return o


def render(dscene, gbuf, camera, sample_count, opt):
    """render() (rt/render.cuh:62): resets when sample_count == 0, then opt.passes passes."""
    check(lib().rt_render(dscene.prepared, gbuf.g, camera, sample_count, ctypes.byref(opt)))


# ---------------------------------------------------------------- ray queries
def query_options(traversal=None, stream=None, stats=None):
    """RtQueryOptions; traversal: TRAVERSAL_BOUNDED (the default) / TRAVERSAL_KD; stream: a hipStream_t as an
    integer (None: synchronous); stats: a device pointer to 3 u64 (rays, hits, rays traced by the plain KD
    traversal; the call adds to them)."""
    o = RtQueryOptions()
    lib().rt_default_query_options(ctypes.byref(o))
    if traversal is not None:
        o.traversal = traversal
    o.stream = stream
    o.stats_device = stats
    return o


class DeviceArray:
    """A device allocation of the C-ABI that knows the shape and dtype of the numpy array it holds.
    DeviceArray(a) uploads a copy of the array `a`; DeviceArray(shape, dtype) is uninitialised, or zeroed with
    zero=True.  `.p` is the c_void_p the *_device calls take; they, and any ctypes call, take the object itself too.
    A context manager: freed on exit.  A zero-size array still owns an allocation; its copies are skipped."""

    def __init__(self, a, dtype=None, zero=False):
        if dtype is None:
            a = np.ascontiguousarray(a)
            self._describe(a.shape, a.dtype)
        else:
            self._describe(a, dtype)
        self.owned = True
        self.p = ctypes.c_void_p()
        check(lib().rt_device_alloc(ctypes.byref(self.p), max(self.nbytes, 16)))
        try:
            if dtype is None:
                self.upload(a)
            elif zero:
                self.zero()
        except BaseException:
            self.free()
            raise

    @classmethod
    def at(cls, p, shape, dtype):
        """device memory someone else owns (a G_Buffer's array, a tensor's data_ptr()) as an array: free() leaves
        it alone"""
        self = cls.__new__(cls)
        self._describe(shape, dtype)
        self.owned, self.p = False, ctypes.c_void_p(_int_ptr(p))
        return self

    def _describe(self, shape, dtype):
        self.shape = (int(shape),) if np.ndim(shape) == 0 else tuple(int(v) for v in shape)
        self.dtype = np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape, dtype=np.int64)) * self.dtype.itemsize

    @property
    def _as_parameter_(self):
        return self.p

    def upload(self, a):
        a = np.ascontiguousarray(a, dtype=self.dtype)
        if a.nbytes != self.nbytes:
            raise ValueError(f"an array of {a.nbytes} bytes does not fill a device array of {self.nbytes}")
        if self.nbytes:
            check(lib().rt_upload(self.p, _ptr(a), self.nbytes))

    def read(self):
        """a new numpy array of the device array's shape and dtype"""
        out = np.empty(self.shape, self.dtype)
        if self.nbytes:
            check(lib().rt_download(_ptr(out), self.p, self.nbytes))
        return out

    def zero(self):
        if self.nbytes:
            check(lib().rt_memset(self.p, 0, self.nbytes))

    def free(self):
        if self.p and self.owned:
            lib().rt_free(self.p)
        self.p = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()
        return False


def _int_ptr(p):
    if isinstance(p, DeviceArray):
        p = p.p
    return p.value if isinstance(p, ctypes.c_void_p) else p


class _Staged(contextlib.ExitStack):
    """the device arrays of one numpy-level call, freed together when it ends"""

    def put(self, a, dtype=None, zero=False):
        return self.enter_context(DeviceArray(a, dtype, zero))

    def put_arrays(self, values):
        """uploads the numpy arrays among `values`; anything else is a device pointer already"""
        return [self.put(a) if isinstance(a, np.ndarray) else a for a in values]

    def stats(self, names, wanted=True):
        """the zeroed block a call adds its counts to — None, for the call too, when they are not wanted"""
        return self.put(len(names), np.uint64, zero=True) if wanted else None


def _stats_dict(names, words):
    return dict(zip(names, (int(v) for v in words)))


def _stats_out(names, block):
    """what a stats block (_Staged.stats) adds to a call's returned tuple"""
    return () if block is None else (_stats_dict(names, block.read()),)


def _synchronize_stream(stream):
    """the numpy path reads the results back at once: wait for the whole device (the downloads that follow
    join the renders anyway, as every rt_download does)"""
    if stream:
        check(lib().rt_synchronize())


def _rays_array(rays):
    rays = np.ascontiguousarray(rays, dtype=np.float32)
    if rays.ndim != 2 or rays.shape[1] != 6:
        raise ValueError("rays must have shape (n, 6)")
    return rays


def _rng_array(rng, n):
    rng = np.asarray(rng)
    if rng.dtype != np.uint32 or rng.shape != (n,):
        raise ValueError("rng must be a uint32 array of shape (n,)")
    return np.ascontiguousarray(rng)


def _sums_to_add(n, radiance, sq, count=None):
    """checks the arrays of an earlier call that an accumulating call adds to (None: not given)"""
    if radiance is None and sq is not None:
        raise ValueError("sq without radiance: pass both arrays of the earlier call to accumulate")
    if count is not None and radiance is None:
        raise ValueError("count array without radiance: pass the arrays of the earlier call to accumulate")
    for name, a, shape, dt in (("radiance", radiance, (n, 3), np.float32), ("sq", sq, (n,), np.float32),
                               ("count", count, (n,), np.int32)):
        if a is not None and (np.asarray(a).dtype != dt or np.asarray(a).shape != shape):
            raise ValueError(f"{name} must be a {np.dtype(dt).name} array of shape {shape}")


def _frame_array(a, dtype, size, what="buffer does not match the frame size"):
    a = np.ascontiguousarray(a, dtype=dtype)
    if a.size != size:
        raise ValueError(what)
    return a


def _opt_ptr(a):
    return None if a is None else _ptr(a)


def trace_rays_device(dscene, rays_ptr, n, hits_ptr, surface_ptr=None, traversal=None, stream=None, stats_ptr=None):
    """rt_trace_rays on device memory: device pointers (integers such as a torch tensor's data_ptr(), or
    DeviceArrays) to n x 6 float32 rays, n RtRayHit (RAY_HIT, 16 B) and optionally n RtRaySurface (RAY_SURFACE,
    80 B); stream: an integer hipStream_t (torch.cuda.current_stream().cuda_stream) — the call is then only
    enqueued."""
    o = query_options(traversal, stream, _int_ptr(stats_ptr))
    check(lib().rt_trace_rays(dscene.prepared, _int_ptr(rays_ptr), int(n), _int_ptr(hits_ptr), _int_ptr(surface_ptr),
                              ctypes.byref(o)))


def trace_rays(dscene, rays, surface=False, traversal=None, stream=None, stats=False):
    """Closest hits of `rays` — a numpy (n, 6) float32 array (origin, direction; directions are used as given,
    not normalised) — bit-identical to the reference's trace_ray.  Returns the RAY_HIT record array
    (triangle -1: miss); with surface=True also the RAY_SURFACE records; with stats=True also a dict of the
    call's counts (QUERY_STATS)."""
    rays = _rays_array(rays)
    n = len(rays)
    with _Staged() as s:
        d_rays, d_hits = s.put(rays), s.put(n, RAY_HIT)
        d_surf = s.put(n, RAY_SURFACE) if surface else None
        d_st = s.stats(QUERY_STATS, stats)
        trace_rays_device(dscene, d_rays, n, d_hits, d_surf, traversal, stream, d_st)
        _synchronize_stream(stream)
        out = (d_hits.read(),) + ((d_surf.read(),) if surface else ()) + _stats_out(QUERY_STATS, d_st)
    return out[0] if len(out) == 1 else out


OCCLUSION_STATS = ("rays", "occluded", "kd_rays")  # rt_occluded's stats_device [0..2]


def occluded_device(dscene, rays_ptr, tmax_ptr, n, out_ptr, traversal=None, stream=None, stats_ptr=None):
    """rt_occluded on device memory: device pointers (as trace_rays_device's) to n x 6 float32 rays, n float32
    tmax (None: +inf for every ray) and n output bytes (any alignment); stream: an integer hipStream_t
    (torch.cuda.current_stream().cuda_stream) — the call is then only enqueued."""
    o = query_options(traversal, stream, _int_ptr(stats_ptr))
    check(lib().rt_occluded(dscene.prepared, _int_ptr(rays_ptr), _int_ptr(tmax_ptr), int(n), _int_ptr(out_ptr),
                            ctypes.byref(o)))


def occluded(dscene, rays, tmax=None, traversal=None, stream=None, stats=False):
    """Whether anything lies on `rays` — a numpy (n, 6) float32 array as for trace_rays — before `tmax` (a
    scalar or an (n,) array in units of the ray parameter; None: +inf): a uint8 array, 1 where the
    reference's trace_ray hits with a ray parameter s < tmax.  With stats=True also a dict of the call's
    counts (OCCLUSION_STATS)."""
    rays = _rays_array(rays)
    n = len(rays)
    if tmax is not None:
        tmax = np.asarray(tmax, dtype=np.float32)
        if tmax.ndim not in (0, 1) or (tmax.ndim == 1 and len(tmax) != n):
            raise ValueError("tmax must be a scalar or have shape (n,)")
        tmax = np.broadcast_to(tmax, (n,))
    with _Staged() as s:
        d_rays, d_out = s.put(rays), s.put(n, np.uint8)
        d_tmax = None if tmax is None else s.put(tmax)
        d_st = s.stats(OCCLUSION_STATS, stats)
        occluded_device(dscene, d_rays, d_tmax, n, d_out, traversal, stream, d_st)
        _synchronize_stream(stream)
        out = (d_out.read(),) + _stats_out(OCCLUSION_STATS, d_st)
    return out if stats else out[0]


PATH_STATS = ("rays", "paths", "trace_calls", "cut_paths", "max_depth")  # RtPathOptions.stats_device [0..4]


def path_options(samples=1, max_depth=0, accumulate=False, traversal=None, stream=None, stats=None):
    """RtPathOptions; samples: paths per ray; max_depth: 0 = unbounded, else the most extension rays of a path;
    accumulate: add to what the output buffers hold; traversal, stream as query_options; stats: a device
    pointer to 5 u64 (PATH_STATS: the call adds to the first four, the fifth is a maximum)."""
    o = RtPathOptions()
    lib().rt_default_path_options(ctypes.byref(o))
    o.samples, o.max_depth, o.accumulate = int(samples), int(max_depth), int(accumulate)
    if traversal is not None:
        o.traversal = traversal
    o.stream = stream
    o.stats_device = stats
    return o


def trace_paths_device(dscene, rays_ptr, rng_ptr, n, radiance_ptr, sq_ptr=None, samples=1, max_depth=0,
                       accumulate=False, traversal=None, stream=None, stats_ptr=None):
    """rt_trace_paths on device memory: device pointers (as trace_rays_device's) to n x 6 float32 rays, n uint32
    RNG states (read and written), n x 3 float32 radiance sums and optionally n float32 sums of squared
    luminance; stream: an integer hipStream_t (torch.cuda.current_stream().cuda_stream) — the call is then only
    enqueued."""
    o = path_options(samples, max_depth, accumulate, traversal, stream, _int_ptr(stats_ptr))
    check(lib().rt_trace_paths(dscene.prepared, _int_ptr(rays_ptr), _int_ptr(rng_ptr), int(n), _int_ptr(radiance_ptr),
                               _int_ptr(sq_ptr), ctypes.byref(o)))


def _put_sums(s, n, radiance, sq):
    """the radiance and sq sums of a path call on the device: the caller's arrays to add to (an absent sq: zeros),
    or uninitialised ones the call writes"""
    if radiance is None:
        return s.put((n, 3), np.float32), s.put(n, np.float32)
    return s.put(radiance), s.put(sq) if sq is not None else s.put(n, np.float32, zero=True)


def trace_paths(dscene, rays, rng, samples=1, max_depth=0, traversal=None, stream=None, stats=False, radiance=None,
                sq=None):
    """Path-traced radiance along `rays` — a numpy (n, 6) float32 array as for trace_rays — `samples` paths
    each, from the (n,) uint32 RNG states `rng`: the reference's trace_path, bit for bit.  Returns (radiance
    (n, 3) float32, sq (n,) float32, rng_out (n,) uint32): the SUMS of L and of luminance(L)^2 over the samples
    and the RNG states after them; with stats=True also a dict of the call's counts (PATH_STATS).  Passing
    `radiance` (and `sq`) arrays of an earlier call accumulates onto them (they are not modified)."""
    rays = _rays_array(rays)
    n = len(rays)
    rng = _rng_array(rng, n)
    _sums_to_add(n, radiance, sq)
    with _Staged() as s:
        d_rays, d_rng = s.put(rays), s.put(rng)
        d_rad, d_sq = _put_sums(s, n, radiance, sq)
        d_st = s.stats(PATH_STATS, stats)
        trace_paths_device(dscene, d_rays, d_rng, n, d_rad, d_sq, samples, max_depth, radiance is not None, traversal,
                           stream, d_st)
        _synchronize_stream(stream)
        return (d_rad.read(), d_sq.read(), d_rng.read()) + _stats_out(PATH_STATS, d_st)


# ---------------------------------------------------------------- path samplers
SAMPLER_PINHOLE, SAMPLER_EQUIRECT, SAMPLER_FISHEYE, SAMPLER_ORTHO, SAMPLER_HEMISPHERE = range(5)
SAMPLER_KINDS = {"pinhole": SAMPLER_PINHOLE, "equirect": SAMPLER_EQUIRECT, "fisheye": SAMPLER_FISHEYE,
                 "ortho": SAMPLER_ORTHO, "hemisphere": SAMPLER_HEMISPHERE}


class Sampler:
    """RtSampler: how rt_sample_paths / rt_sampler_rays draw each element's rays (include/isaklm_rt.h has the
    definition of every kind).  kind: a SAMPLER_* value or its name.  Image kinds take width, height and a Camera
    (FISHEYE: camera.FOV is the full angle across the image circle; ORTHO: ortho_half_width), and optionally
    `pixels`, an int32 array of pixel indices y * width + x (out-of-range entries give rays that hit nothing);
    HEMISPHERE takes `points`, an (n, 6) float32 array of positions and normals."""

    def __init__(self, kind, width=0, height=0, camera=None, ortho_half_width=0.0, pixels=None, points=None):
        self.kind = SAMPLER_KINDS[kind] if isinstance(kind, str) else int(kind)
        self.width, self.height = int(width), int(height)
        self.camera = camera if camera is not None else Camera()
        self.ortho_half_width = float(ortho_half_width)
        self.pixels = None if pixels is None else np.ascontiguousarray(pixels, dtype=np.int32).reshape(-1)
        self.points = None
        if points is not None:
            self.points = np.ascontiguousarray(points, dtype=np.float32)
            if self.points.ndim != 2 or self.points.shape[1] != 6:
                raise ValueError("points must have shape (n, 6)")

    @property
    def n(self):
        """the number of elements: the points, the listed pixels, or the whole frame"""
        if self.kind == SAMPLER_HEMISPHERE:
            return 0 if self.points is None else len(self.points)
        return self.width * self.height if self.pixels is None else len(self.pixels)

    def struct(self, pixels_ptr=None, points_ptr=None):
        """the RtSampler with the given pointers to its pixel list / points (device or host, as the call wants)"""
        return RtSampler(self.kind, self.width, self.height, self.camera, self.ortho_half_width, _int_ptr(pixels_ptr),
                         _int_ptr(points_ptr))


def _sampler_lists(sampler, put):
    """(pixels, points) of a Sampler as a call takes them: `put` makes an array's pointer (an upload, or the host
    array's own).  An empty list still is a list: the call sees the non-null dummies 4 and 8 (n == 0 is answered
    before a pointer is looked at)."""
    return [None if a is None else put(a) if a.size else dummy
            for a, dummy in ((sampler.pixels, 4), (sampler.points, 8))]


def sample_paths_device(dscene, sampler, rng_ptr, n, radiance_ptr, sq_ptr=None, count_ptr=None, samples=1, max_depth=0,
                        accumulate=False, traversal=None, stream=None, stats_ptr=None, pixels_ptr=None,
                        points_ptr=None, adaptive=None):
    """rt_sample_paths on device memory: `sampler` a Sampler (its arrays are not used: pixels_ptr / points_ptr
    are the device pointers to them); device pointers (as trace_rays_device's) to n uint32 RNG states (read and
    written), n x 3 float32 radiance sums, optionally n float32 sums of squared luminance and n int32 sample
    counts — a G_Buffer's four arrays, for a whole frame; stream: an integer hipStream_t — the call is then only
    enqueued.  adaptive=(min_samples, tolerance): rt_sample_paths_adaptive — the renderer's adaptive test before
    every sample (sq_ptr and count_ptr are then required)."""
    o = path_options(samples, max_depth, accumulate, traversal, stream, _int_ptr(stats_ptr))
    smp = sampler.struct(pixels_ptr, points_ptr)
    args = (dscene.prepared, ctypes.byref(smp), _int_ptr(rng_ptr), int(n), _int_ptr(radiance_ptr), _int_ptr(sq_ptr),
            _int_ptr(count_ptr), ctypes.byref(o))
    if adaptive is None:
        check(lib().rt_sample_paths(*args))
    else:
        ad = RtAdaptive(int(adaptive[0]), float(adaptive[1]))
        check(lib().rt_sample_paths_adaptive(*args, ctypes.byref(ad)))


def sample_paths(dscene, sampler, rng, samples=1, max_depth=0, traversal=None, stream=None, stats=False,
                 radiance=None, sq=None, count=None, adaptive=None):
    """Path-traced radiance of `samples` rays per element drawn by `sampler` (a Sampler) on the device from the
    (n,) uint32 RNG states `rng`.  Returns (radiance (n, 3) float32, sq (n,) float32, rng_out (n,) uint32): the
    SUMS over the samples, as trace_paths; with count=True also the (n,) int32 sample counts; with stats=True
    also a dict of the call's counts (PATH_STATS).  Passing `radiance` (with `sq`, and `count` as an int32 array)
    of an earlier call accumulates onto them (they are not modified).  adaptive=(min_samples, tolerance): the
    renderer's adaptive test before every sample (rt_sample_paths_adaptive) — an element takes at most `samples`
    samples; the counts are then always returned (count=True is implied), and accumulating needs all three arrays."""
    if adaptive is not None:
        if radiance is not None and (sq is None or count is None or isinstance(count, bool)):
            raise ValueError("adaptive accumulation needs the radiance, sq and count arrays of the earlier call")
        if count is None or count is False:
            count = True
    n = sampler.n
    rng = _rng_array(rng, n)
    want_count = count is not None and count is not False
    count_arr = None if count is None or isinstance(count, bool) else np.asarray(count)
    _sums_to_add(n, radiance, sq, count_arr)
    accumulate = radiance is not None
    with _Staged() as s:
        d_pix, d_pts = _sampler_lists(sampler, s.put)
        d_rng = s.put(rng)
        d_rad, d_sq = _put_sums(s, n, radiance, sq)
        d_cnt = None
        if want_count:
            d_cnt = s.put(count_arr) if count_arr is not None else s.put(n, np.int32, zero=accumulate)
        d_st = s.stats(PATH_STATS, stats)
        sample_paths_device(dscene, sampler, d_rng, n, d_rad, d_sq, d_cnt, samples, max_depth, accumulate, traversal,
                            stream, d_st, d_pix, d_pts, adaptive)
        _synchronize_stream(stream)
        return (d_rad.read(), d_sq.read(), d_rng.read()) + ((d_cnt.read(),) if want_count else ()) + \
            _stats_out(PATH_STATS, d_st)


CONVERGENCE_STATS = ("elements", "open", "below_min", "samples")  # rt_convergence's stats [0..3]


def convergence_device(radiance_ptr, sq_ptr, count_ptr, n, min_samples, tolerance, rel_error_ptr=None, stats_ptr=None,
                       stream=None):
    """rt_convergence on device memory: device pointers (as trace_rays_device's) to n x 3 float32 radiance sums,
    n float32 sums of squared luminance and n int32 sample counts (a G_Buffer's arrays, or sample_paths'
    outputs); optionally n float32 for the relative-error map and 4 u64 the call adds CONVERGENCE_STATS to."""
    check(lib().rt_convergence(_int_ptr(radiance_ptr), _int_ptr(sq_ptr), _int_ptr(count_ptr), int(n), int(min_samples),
                               float(tolerance), _int_ptr(rel_error_ptr), _int_ptr(stats_ptr), stream))


def _convergence_arrays(radiance, sq, count):
    radiance = np.ascontiguousarray(radiance, dtype=np.float32)
    sq = np.ascontiguousarray(sq, dtype=np.float32).reshape(-1)
    count = np.ascontiguousarray(count, dtype=np.int32).reshape(-1)
    n = len(count)
    if radiance.size != 3 * n or sq.size != n:
        raise ValueError("radiance must hold n x 3, sq and count n values")
    return radiance.reshape(n, 3), sq, count, n


def convergence(radiance, sq, count, min_samples, tolerance, rel_error=False):
    """rt_convergence on numpy arrays (uploaded for the call): a dict of CONVERGENCE_STATS — `open` is the number
    of elements the adaptive test would sample on the next pass, 0 = converged; with rel_error=True also the (n,)
    float32 relative-error map."""
    radiance, sq, count, n = _convergence_arrays(radiance, sq, count)
    with _Staged() as s:
        d_err = s.put(n, np.float32) if rel_error and n else None
        d_st = s.stats(CONVERGENCE_STATS)
        convergence_device(s.put(radiance), s.put(sq), s.put(count), n, min_samples, tolerance, d_err, d_st)
        stats = _stats_dict(CONVERGENCE_STATS, d_st.read())
        return (stats, d_err.read() if d_err is not None else np.zeros(0, np.float32)) if rel_error else stats


def convergence_host(radiance, sq, count, min_samples, tolerance, rel_error=False):
    """rt_convergence_host: convergence computed on the host, bit for bit (no GPU is touched)."""
    radiance, sq, count, n = _convergence_arrays(radiance, sq, count)
    st = np.zeros(4, dtype=np.uint64)
    err = np.zeros(max(n, 1), dtype=np.float32)
    check(lib().rt_convergence_host(_ptr(radiance), _ptr(sq), _ptr(count), n, int(min_samples), float(tolerance),
                                    _ptr(err) if rel_error else None, _ptr(st)))
    stats = _stats_dict(CONVERGENCE_STATS, st)
    return (stats, err[:n]) if rel_error else stats


def sampler_rays(sampler, rng=None):
    """rt_sampler_rays: one sample's rays of every element of `sampler`, drawn on the device from the (n,) uint32
    RNG states `rng`: (rays (n, 6) float32, rng_out).  rng None: the centre rays (image kinds), rays alone."""
    n = sampler.n
    rng = None if rng is None else _rng_array(rng, n)
    with _Staged() as s:
        smp = sampler.struct(*_sampler_lists(sampler, s.put))
        d_rng = None if rng is None else s.put(rng)
        d_rays = s.put((n, 6), np.float32)
        check(lib().rt_sampler_rays(ctypes.byref(smp), d_rng, n, d_rays, None))
        return d_rays.read() if rng is None else (d_rays.read(), d_rng.read())


def sampler_rays_host(sampler, rng=None):
    """rt_sampler_rays_host: sampler_rays computed on the host, bit for bit (no GPU is touched)."""
    n = sampler.n
    rng = None if rng is None else _rng_array(rng, n).copy()
    rays = np.zeros((max(n, 1), 6), dtype=np.float32)
    smp = sampler.struct(*_sampler_lists(sampler, _ptr))
    check(lib().rt_sampler_rays_host(ctypes.byref(smp), _opt_ptr(rng), n, _ptr(rays)))
    rays = rays[:n]
    return rays if rng is None else (rays, rng)


def camera_rays(camera, width, height):
    """rt_camera_rays: the (width*height, 6) float32 pixel-centre rays of `camera` (ray y*width + x, row 0 =
    bottom): the renderer's camera ray with both jitter draws 0.5 and no aperture offset."""
    with DeviceArray((width * height, 6), np.float32) as d:
        check(lib().rt_camera_rays(camera, width, height, d, None))
        return d.read()


# the first-hit feature buffers (RtAovBuffers' order): name -> (dtype, values per pixel)
_AOVS = {"depth": (np.float32, 1), "normal": (np.float32, 3), "albedo": (np.float32, 3), "triangle": (np.int32, 1)}


def _aov_buffers(depth, normal, albedo, triangle):
    return RtAovBuffers(_int_ptr(depth), _int_ptr(normal), _int_ptr(albedo), _int_ptr(triangle))


def _put_aov_outputs(s, lead):
    """the four AOV arrays of a frame or pixel list of shape `lead` on the device: {name: DeviceArray}"""
    return {k: s.put(lead + ((per,) if per > 1 else ()), dtype) for k, (dtype, per) in _AOVS.items()}


def _aov_inputs(aov, names, W, H):
    """aov's entries for `names` as a device call takes them: a numpy array, checked against the frame, is to be
    uploaded for the call (_Staged.put_arrays); anything else is a device pointer already (None: no such buffer)"""
    return [_frame_array(aov[k], _AOVS[k][0], W * H * _AOVS[k][1], f"aov[{k!r}] does not match the {W} x {H} frame")
            if isinstance(aov.get(k), np.ndarray) else aov.get(k) for k in names]


def render_aov(dscene, camera, width, height, traversal=None):
    """rt_render_aov: the first-hit feature buffers of the pixel-centre rays, as a dict of numpy arrays with
    row 0 = bottom: depth (H, W) float32 (inf: miss), normal and albedo (H, W, 3) float32, triangle (H, W)
    int32 (-1: miss)."""
    with _Staged() as s:
        d = _put_aov_outputs(s, (height, width))
        b = _aov_buffers(*d.values())
        o = query_options(traversal)
        check(lib().rt_render_aov(dscene.prepared, camera, width, height, ctypes.byref(b), ctypes.byref(o)))
        return {k: a.read() for k, a in d.items()}


def sample_aov_device(dscene, sampler, n, aov_ptrs, traversal=None, stream=None, stats_ptr=None, pixels_ptr=None):
    """rt_sample_aov on device memory: `sampler` a Sampler (its pixel array is not used: pixels_ptr is the device
    pointer to it), aov_ptrs (depth, normal, albedo, triangle) device pointers, any of them None."""
    b = _aov_buffers(*aov_ptrs)
    o = query_options(traversal, stream, _int_ptr(stats_ptr))
    smp = sampler.struct(pixels_ptr, None)
    check(lib().rt_sample_aov(dscene.prepared, ctypes.byref(smp), int(n), ctypes.byref(b), ctypes.byref(o)))


def sample_aov(dscene, sampler, traversal=None, stats=False):
    """rt_sample_aov: the first-hit feature buffers of an image sampler's centre rays, render_aov's dict — shaped
    (H, W, ...) with row 0 = bottom for a whole frame, (n, ...) for a pixel list (out-of-frame entries miss: depth
    inf, triangle -1); with stats=True also a dict of the call's counts (QUERY_STATS)."""
    n = sampler.n
    with _Staged() as s:
        d_pix, _ = _sampler_lists(sampler, s.put)
        d = _put_aov_outputs(s, (sampler.height, sampler.width) if sampler.pixels is None else (n,))
        d_st = s.stats(QUERY_STATS, stats)
        sample_aov_device(dscene, sampler, n, list(d.values()), traversal, None, d_st, d_pix)
        out = ({k: a.read() for k, a in d.items()},) + _stats_out(QUERY_STATS, d_st)
    return out if stats else out[0]


def _frame_sampler_struct(sampler):
    """the RtSampler of a whole-frame call: a pixel list stays visible to the library (which refuses it) without
    being uploaded"""
    return sampler.struct(None if sampler.pixels is None else 4, None if sampler.points is None else 8)


def _frame_entry(call, host, samplers, views, size):
    """(entry point, view arguments, size arguments) of a frame call and its host twin (host "_host"): `call` takes
    its views (Cameras; a None is no view) as they are and the frame's size; for whole-frame Samplers
    `call`_sampler takes pointers to their RtSamplers and no size.  Resolves rt_denoise, rt_denoise_host,
    rt_denoise_sampler, rt_denoise_sampler_host, rt_reproject, rt_reproject_host, rt_reproject_sampler and
    rt_reproject_sampler_host."""
    if not samplers:
        return getattr(lib(), call + host), [v for v in views if v is not None], list(size)
    return getattr(lib(), call + "_sampler" + host), [ctypes.byref(_frame_sampler_struct(v)) for v in views], []


# ---------------------------------------------------------------- denoising
def denoise_options(iterations=0, sigma_lum=0.0, sigma_depth=0.0, normal_log2=0, demodulate=True, stream=None):
    """RtDenoiseOptions; 0 = the library default (5 levels, sigma_lum 4, sigma_depth 1, normal_log2 7);
    demodulate False filters the colour itself (no albedo needed); stream: an integer hipStream_t."""
    o = RtDenoiseOptions()
    o.iterations, o.sigma_lum, o.sigma_depth, o.normal_log2 = iterations, sigma_lum, sigma_depth, normal_log2
    o.demodulate = 1 if demodulate else -1
    o.stream = stream
    return o


def _denoise_device(g, aov_ptrs, sampler, width, height, out_ptr, options):
    """rt_denoise_sampler for a Sampler's frame, rt_denoise (sampler None) for a width x height one"""
    b = _aov_buffers(aov_ptrs[0], aov_ptrs[1], aov_ptrs[2], None)
    o = denoise_options(**options)
    fn, view, size = _frame_entry("rt_denoise", "", sampler is not None, [sampler], (width, height))
    check(fn(g, ctypes.byref(b), *view, *size, _int_ptr(out_ptr), ctypes.byref(o)))


def denoise_device(g, aov_ptrs, width, height, out_ptr, **options):
    """rt_denoise on device memory: g a G_Buffer struct, aov_ptrs (depth, normal, albedo) device pointers
    (integers or DeviceArrays; albedo may be None with demodulate=False), out_ptr width*height*3 floats."""
    _denoise_device(g, aov_ptrs, None, width, height, out_ptr, options)


def denoise_sampler_device(g, aov_ptrs, sampler, out_ptr, **options):
    """rt_denoise_sampler on device memory: denoise_device with a Sampler (a whole frame of an image kind) in place
    of width and height; an equirect sampler's x axis is periodic."""
    _denoise_device(g, aov_ptrs, sampler, 0, 0, out_ptr, options)


def denoise(gbuf, aov, **options):
    """rt_denoise: the denoised mean radiance of `gbuf` as (H, W, 3) float32, row 0 = bottom.  aov: the dict
    rt.render_aov returns (numpy arrays, uploaded here) or a dict of device pointers; keys depth, normal and —
    unless demodulate=False — albedo.  Options: denoise_options."""
    return _denoise(gbuf, aov, None, options)


def denoise_sampler(gbuf, aov, sampler, **options):
    """rt_denoise_sampler: denoise for the frame of `sampler` (a Sampler of an image kind without a pixel list,
    gbuf's size); aov: the dict rt.sample_aov returns, or device pointers.  For every kind but equirect the
    result is denoise's; an equirect frame is filtered across the seam at longitude +-pi."""
    if (sampler.width, sampler.height) != (gbuf.width, gbuf.height):
        raise ValueError("the sampler's frame is not the G-buffer's")
    return _denoise(gbuf, aov, sampler, options)


def _denoise(gbuf, aov, sampler, options):
    W, H = gbuf.width, gbuf.height
    guides = _aov_inputs(aov, ("depth", "normal", "albedo"), W, H)
    with _Staged() as s:
        d_out = s.put((H, W, 3), np.float32)
        _denoise_device(gbuf.g, s.put_arrays(guides), sampler, W, H, d_out, options)
        _synchronize_stream(options.get("stream"))
        return d_out.read()


def denoise_host(fb, sq, count, depth, normal, albedo, **options):
    """rt_denoise_host: rt_denoise's arithmetic on the CPU, bit-identical to the GPU.  fb (H, W, 3), sq and
    count (H, W), depth (H, W), normal and albedo (H, W, 3) (albedo may be None with demodulate=False); the
    frame size is taken from depth's shape.  Returns (H, W, 3) float32."""
    return _denoise_host(fb, sq, count, depth, normal, albedo, None, options)


def denoise_sampler_host(fb, sq, count, depth, normal, albedo, sampler, **options):
    """rt_denoise_sampler_host: denoise_host for the frame of `sampler` (the arrays must have its size),
    bit-identical to denoise_sampler."""
    return _denoise_host(fb, sq, count, depth, normal, albedo, sampler, options)


def _host_frame(depth, sampler, what):
    """(depth as a float32 array, W, H) of a host twin's frame, which is `sampler`'s if one is given"""
    depth = np.ascontiguousarray(depth, dtype=np.float32)
    if depth.ndim != 2:
        raise ValueError("depth must have shape (H, W)")
    H, W = depth.shape
    if sampler is not None and (sampler.width, sampler.height) != (W, H):
        raise ValueError(what)
    return depth, W, H


def _denoise_host(fb, sq, count, depth, normal, albedo, sampler, options):
    depth, W, H = _host_frame(depth, sampler, "the sampler's frame is not the arrays'")
    n = W * H
    arrays = [_frame_array(fb, np.float32, 3 * n), _frame_array(sq, np.float32, n), _frame_array(count, np.int32, n),
              depth, _frame_array(normal, np.float32, 3 * n),
              None if albedo is None else _frame_array(albedo, np.float32, 3 * n)]
    out = np.zeros((H, W, 3), np.float32)
    o = denoise_options(**options)
    fn, view, size = _frame_entry("rt_denoise", "_host", sampler is not None, [sampler], (W, H))
    check(fn(*[_opt_ptr(a) for a in arrays], *view, *size, _ptr(out), ctypes.byref(o)))
    return out


# ---------------------------------------------------------------- temporal reprojection
REPROJECT_STATS = ("pixels", "kept_pixels", "carried_samples")  # RtReprojectOptions.stats_device [0..2]


def reproject_options(max_history=0, depth_tol=0.0, normal_min=0.0, match_triangle=True, stream=None, stats=None):
    """RtReprojectOptions; 0 = the library default (max_history 64, depth_tol 0.02, normal_min 0.95);
    match_triangle False carries history across triangle edges of one surface; stream: an integer hipStream_t;
    stats: a device pointer to 3 u64 (REPROJECT_STATS; the call adds to them)."""
    o = RtReprojectOptions()
    o.max_history, o.depth_tol, o.normal_min = int(max_history), depth_tol, normal_min
    o.match_triangle = 1 if match_triangle else -1
    o.stream = stream
    o.stats_device = stats
    return o


def _reproject_device(g_src, aov_src_ptrs, view_src, aov_dst_ptrs, view_dst, size, g_dst, options):
    """rt_reproject for two Cameras and a (width, height) size, rt_reproject_sampler (size None) for two Samplers"""
    bs, bd = (_aov_buffers(p[0], p[1], None, p[2]) for p in (aov_src_ptrs, aov_dst_ptrs))
    if "stats" in options:
        options = dict(options, stats=_int_ptr(options["stats"]))
    o = reproject_options(**options)
    fn, (src, dst), size = _frame_entry("rt_reproject", "", size is None, (view_src, view_dst), size or ())
    check(fn(g_src, ctypes.byref(bs), src, ctypes.byref(bd), dst, *size, g_dst, ctypes.byref(o)))


def reproject_device(g_src, aov_src_ptrs, cam_src, aov_dst_ptrs, cam_dst, width, height, g_dst, **options):
    """rt_reproject on device memory: g_src, g_dst G_Buffer structs, aov_*_ptrs (depth, normal, triangle)
    device pointers (integers or DeviceArrays; triangle may be None)."""
    _reproject_device(g_src, aov_src_ptrs, cam_src, aov_dst_ptrs, cam_dst, (width, height), g_dst, options)


def reproject_sampler_device(g_src, aov_src_ptrs, smp_src, aov_dst_ptrs, smp_dst, g_dst, **options):
    """rt_reproject_sampler on device memory: reproject_device with two Samplers (whole frames of one image kind
    and size) in place of the two cameras and the frame size."""
    _reproject_device(g_src, aov_src_ptrs, smp_src, aov_dst_ptrs, smp_dst, None, g_dst, options)


def reproject_sampler(gbuf_src, aov_src, smp_src, aov_dst, smp_dst, out=None, stats=False, **options):
    """rt_reproject_sampler: reproject for a moved camera of any image kind — smp_src, smp_dst: the Samplers the
    two frames were made with (one kind and size, no pixel lists), aov_src, aov_dst: rt.sample_aov's dicts for
    them.  Returns what reproject returns."""
    if (smp_src.width, smp_src.height) != (gbuf_src.width, gbuf_src.height):
        raise ValueError("the source sampler's frame is not the G-buffer's")
    return _reproject(gbuf_src, aov_src, smp_src, aov_dst, smp_dst, out, stats, options, True)


def reproject(gbuf_src, aov_src, cam_src, aov_dst, cam_dst, out=None, stats=False, **options):
    """rt_reproject: carries gbuf_src (rendered at cam_src) over to cam_dst.  aov_src, aov_dst: the dicts
    rt.render_aov returns for the two cameras (numpy arrays, uploaded here) or dicts of device pointers; keys
    depth, normal and optionally triangle.  Fills `out` (its RNG states are left alone) or returns a new
    GBuffer whose RNG states are gbuf_src's, so the per-pixel streams continue; with stats=True returns (gbuf,
    dict of REPROJECT_STATS).  Options: reproject_options."""
    return _reproject(gbuf_src, aov_src, cam_src, aov_dst, cam_dst, out, stats, options, False)


def _reproject(gbuf_src, aov_src, view_src, aov_dst, view_dst, out, stats, options, samplers):
    W, H = gbuf_src.width, gbuf_src.height
    if out is not None and (out.width, out.height) != (W, H):
        raise ValueError("out does not match the source frame's size")
    sides = [_aov_inputs(aov, ("depth", "normal", "triangle"), W, H) for aov in (aov_src, aov_dst)]
    if out is None:
        out = GBuffer(W, H)
        out.array("random_numbers").upload(gbuf_src.array("random_numbers").read())
    with _Staged() as s:
        d_st = s.stats(REPROJECT_STATS, stats)
        if stats:
            options = dict(options, stats=d_st)
        _reproject_device(gbuf_src.g, s.put_arrays(sides[0]), view_src, s.put_arrays(sides[1]), view_dst,
                          None if samplers else (W, H), out.g, options)
        _synchronize_stream(options.get("stream"))
        return (out,) + _stats_out(REPROJECT_STATS, d_st) if stats else out


def reproject_host(src_fb, src_sq, src_count, aov_src, cam_src, aov_dst, cam_dst, stats=False, **options):
    """rt_reproject_host: rt_reproject's arithmetic on the CPU, bit-identical to the GPU.  src_fb (H, W, 3),
    src_sq and src_count (H, W); aov_src, aov_dst: dicts with depth (H, W), normal (H, W, 3) and optionally
    triangle (H, W); the frame size is taken from aov_dst's depth.  Returns (fb (H, W, 3) float32, sq (H, W)
    float32, count (H, W) int32), with stats=True also a dict of REPROJECT_STATS."""
    return _reproject_host(src_fb, src_sq, src_count, aov_src, cam_src, aov_dst, cam_dst, stats, options, False)


def reproject_sampler_host(src_fb, src_sq, src_count, aov_src, smp_src, aov_dst, smp_dst, stats=False, **options):
    """rt_reproject_sampler_host: reproject_host with two Samplers in place of the two cameras (the arrays must have
    their frame's size), bit-identical to reproject_sampler."""
    return _reproject_host(src_fb, src_sq, src_count, aov_src, smp_src, aov_dst, smp_dst, stats, options, True)


def _reproject_host(src_fb, src_sq, src_count, aov_src, view_src, aov_dst, view_dst, stats, options, samplers):
    _, W, H = _host_frame(aov_dst["depth"], view_dst if samplers else None,
                          "the destination sampler's frame is not the arrays'")
    n = W * H
    sums = [_frame_array(src_fb, np.float32, 3 * n), _frame_array(src_sq, np.float32, n),
            _frame_array(src_count, np.int32, n)]
    sides = [[_frame_array(aov[k], _AOVS[k][0], n * _AOVS[k][1]) for k in ("depth", "normal")] +
             [None if aov.get("triangle") is None else _frame_array(aov["triangle"], np.int32, n)]
             for aov in (aov_src, aov_dst)]
    out = (np.zeros((H, W, 3), np.float32), np.zeros((H, W), np.float32), np.zeros((H, W), np.int32))
    st = np.zeros(3, dtype=np.uint64)
    options.pop("stream", None)
    o = reproject_options(**options)
    sums_p, src, dst = ([_opt_ptr(a) for a in arrays] for arrays in (sums, sides[0], sides[1]))
    tail = [_ptr(a) for a in out] + [_ptr(st), ctypes.byref(o)]
    fn, (v_src, v_dst), size = _frame_entry("rt_reproject", "_host", samplers, (view_src, view_dst), (W, H))
    check(fn(*sums_p, *src, v_src, *dst, v_dst, *size, *tail))
    return out + (_stats_dict(REPROJECT_STATS, st),) if stats else out


def tonemap_rgb(rgb):
    """rt_tonemap_rgb: rt_tonemap's colour math on an (H, W, 3) float32 mean-radiance image (e.g. denoise's
    result) -> (H*W, 4) uint8, row 0 = bottom."""
    rgb = np.ascontiguousarray(rgb, dtype=np.float32)
    H, W = rgb.shape[0], rgb.shape[1]
    with DeviceArray(rgb) as d_rgb, DeviceArray((W * H, 4), np.uint8) as d_out:
        check(lib().rt_tonemap_rgb(d_rgb, d_out, W, H, None))
        return d_out.read()


class DeviceCounters:
    def __init__(self):
        self.words = DeviceArray(N_COUNTERS, np.uint64, zero=True)  # (.read(): the raw counter words)
        self.p = self.words.p

    def zero(self):
        self.words.zero()

    def read(self, finisher=False):
        """The reference-comparable counters; finisher=True adds the wavefront
        finisher's share of node/tri/ray (RT_CNT_FIN_*)."""
        a = self.words.read()
        out = {k: int(a[i]) for i, k in enumerate(COUNTER_NAMES)}
        out["deep_push"] = int(a[15])  # RT_CNT_DEEP_PUSH: reference-comparable (the oracle counts it too)
        if finisher:
            out.update({k: int(a[10 + i]) for i, k in enumerate(FINISH_COUNTER_NAMES) if k})
        return out

    def __del__(self):
        try:
            self.words.free()
        except Exception:
            pass


def tonemap(gbuf):
    """draw_frame colour math -> (H*W, 4) uint8, row 0 = bottom."""
    with DeviceArray((gbuf.n, 4), np.uint8) as d:
        check(lib().rt_tonemap(gbuf.g, d, gbuf.width, gbuf.height, None))
        return d.read()


def save_render(gbuf, path):
    check(lib().rt_save_render(gbuf.g, gbuf.width, gbuf.height, path.encode()))


COMM_ID_BYTES = 128


class Comm:
    """RCCL communicator of the C-ABI (rt_comm_*): rt_reduce_shards sums the
    shards' fb / sq / count into `root`."""

    @staticmethod
    def unique_id():
        buf = ctypes.create_string_buffer(COMM_ID_BYTES)
        check(lib().rt_comm_unique_id(buf))
        return buf.raw

    def __init__(self, nranks, rank, uid):
        L = lib()
        L.rt_comm_create.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_char_p, ctypes.POINTER(ctypes.c_void_p)]
        L.rt_comm_destroy.argtypes = [ctypes.c_void_p]
        L.rt_reduce_shards.argtypes = [ctypes.c_void_p, G_Buffer, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                       ctypes.c_void_p]
        self.h = ctypes.c_void_p()
        check(L.rt_comm_create(nranks, rank, uid, ctypes.byref(self.h)))

    def reduce(self, gbuf_g, width, height, root=0, stream=None):
        check(lib().rt_reduce_shards(self.h, gbuf_g, width, height, root, stream))

    def close(self):
        if self.h:
            check(lib().rt_comm_destroy(self.h))
            self.h = ctypes.c_void_p()
