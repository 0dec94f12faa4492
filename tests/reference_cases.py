"""The cases whose results the reference's own source recorded in
tests/golden/reference/ (one .npz each, written by
tests/golden/make_reference_golden.py from oracle/_ref/libref_rt.so), and the
code that rebuilds a case's inputs and runs it — on the live reference, on the
oracle (both: tests/test_reference_cpu.py) or on the GPU
(tests/test_gpu_reference.py, which reads the fixtures only).

A case is its scene (built by the project's own scene builders into a given
directory), a camera, the frame size, the passes of each call, the sampling
options and the G-buffer seeds.  A fixture holds those inputs, a SHA-256 of
every scene input file (so that a drift in hazards.py, helpers.py or scenes.cpp
is reported as a drift of the inputs and not as a kernel bug), the reference's
scene as hashes (triangles, KD nodes, indices) with its light list and bounds,
and the reference's four G-buffer arrays after each call — or, for the ray
case, the rays and the reference's Samples.
"""
import hashlib
import json
import os

import numpy as np

import hazards
import helpers

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN_DIR = os.path.join(HERE, "golden", "reference")
G_NAMES = ("frame_buffer", "squared_luminance", "sample_count", "random_numbers")
W, H = 48, 36  # multiples of the reference's 3x3 screen cell: path_tracing() has no bounds guard


def _cornell(d):
    return helpers.scene_path("cornell")


def _aligned(d, camera=None):
    return hazards.cornell_variant(d, "aligned", yaw_room=0.0, camera=camera)


def _textured(d):
    return helpers.make_textured_scene(d)[0]


# name -> (scene builder, options).  options: passes (of each call), adaptive, min_samples, size, and how the
# camera and the seeds are made ("camera": "h5" = on the KD root split; "seeds": "h7" / "h4", see hazards.py)
FRAME_CASES = {
    "cornell": (_cornell, {"passes": [4, 4]}),  # two calls: reset, then continue
    "cornell_adaptive": (_cornell, {"passes": [24], "adaptive": True, "min_samples": 4}),
    "aligned": (_aligned, {"passes": [4]}),  # hits on leaf exits (H6)
    "aligned_h5": (_aligned, {"passes": [2], "camera": "h5"}),  # camera on the root split (H5)
    "aligned_axis": (lambda d: _aligned(d, hazards.AXIS_CAMERA), {"passes": [2], "seeds": "h7"}),  # axis-parallel rays
    "degenerate": (lambda d: hazards.cornell_variant(d, "degenerate", extra_obj=hazards.DEGENERATE_OBJ),
                   {"passes": [3]}),  # zero-area triangles (H7)
    "duplicate": (lambda d: hazards.cornell_variant(d, "duplicate", extra_obj=hazards.DUPLICATE_OBJ),
                  {"passes": [3]}),  # ties between identical triangles
    "h4": (_cornell, {"passes": [3], "seeds": "h4", "size": (24, 18)}),  # light pick with xi = 1 (H4)
    "adversarial_near": (lambda d: hazards.adversarial_scene(d, "near"), {"passes": [4]}),
    "adversarial_far": (lambda d: hazards.adversarial_scene(d, "far"), {"passes": [4]}),
    "adversarial_tiny": (lambda d: hazards.adversarial_scene(d, "tiny"), {"passes": [4]}),
    "textured": (_textured, {"passes": [4]}),  # stb decode, UV wrap, the padded texel (H10)
    "trap": (helpers.make_trap_scene, {"passes": [4]}),  # deep paths (wf_long, the deep bounded traversal)
    "features": (lambda d: os.path.join(HERE, "golden", "features", "scene.txt"), {"passes": [4]}),
    "cornell_blob": (lambda d: helpers.scene_path("cornell_blob"), {"passes": [4]}),  # wide BVH, T* certificate
    "materials": (hazards.materials_scene, {"passes": [4, 4]}),  # the BSDF's extremes, one box each; finite frames
}
# Frames with NaN and Inf in them (emittance and albedo of 3e38; roughness, n and k of 1e30; n of 0).  Kept out of
# FRAME_CASES: what loops over that compares bit-strictly, and a NaN's payload and sign are outside the parity
# claim (same_bits here, helpers.assert_same_class on the GPU side: a NaN equals any NaN, all else bit for bit).
NONFINITE_CASES = {
    "materials_nonfinite": (hazards.materials_nonfinite_scene, {"passes": [3, 3], "adaptive": True, "min_samples": 2}),
}
RENDER_CASES = {**FRAME_CASES, **NONFINITE_CASES}
RAY_CASE = "rays_cornell"
RAY_KINDS = (("split", 512), ("axis", 512), ("special", 64), ("inbox", 512))  # test_gpu_query.make_rays' classes
TRAP_MIN_DEPTH = 256  # the trap's deepest path must be at least this (419 when the fixtures were made)
MATERIALS_MIN_DEPTH = 48  # the materials case's deepest path must be at least this (80 when recorded): wf_long
ALL_CASES = list(RENDER_CASES) + [RAY_CASE]


def fixture_path(name):
    return os.path.join(GOLDEN_DIR, name + ".npz")


def load_fixture(name):
    with np.load(fixture_path(name), allow_pickle=False) as z:
        fx = {k: z[k] for k in z.files}
    fx["meta"] = json.loads(str(fx["meta"]))
    return fx


# ------------------------------------------------------------------ inputs
def scene_input_files(scene_path):
    """every file the loaders read for a scene: the scene file, its meshes, their material files and the
    texture files those name (the ones that exist), as (name relative to the scene's directory, path)"""
    d = os.path.dirname(os.path.abspath(scene_path))
    rel = [os.path.basename(scene_path)]
    for line in open(scene_path).read().splitlines():
        t = line.split()
        if t and t[0] == "mesh":
            rel += [t[1], t[2]]
            for ml in open(os.path.join(d, t[2])).read().splitlines():
                mt = ml.split()
                if len(mt) > 1 and mt[0] == "texture" and os.path.exists(os.path.join(d, mt[1])):
                    rel.append(mt[1])
    return [(r, os.path.join(d, r)) for r in sorted(set(rel))]


def file_hashes(scene_path):
    return {r: hashlib.sha256(open(p, "rb").read()).hexdigest() for r, p in scene_input_files(scene_path)}


def register_textures(scene_path):
    """give the oracle the texels of the scene's textures (it decodes no images); decoded by the product's
    decoder, which tests/test_textures.py pins to the reference's stb_image"""
    import oracle
    import rt

    d = os.path.dirname(os.path.abspath(scene_path))
    for r, p in scene_input_files(scene_path):
        if r.lower().endswith((".png", ".jpg", ".jpeg")):
            oracle.register_texture(r, rt.decode_image(os.path.join(d, r)))


class Case:
    """One case's inputs, rebuilt from the project's scene builders into directory d.  `scene` is any loaded
    scene of it (oracle.OracleScene or reference.ReferenceScene: the H5 camera needs the KD root split).
    The H4 seeds are searched for with the oracle's hazard counter (hazards.h4_seeds)."""

    def __init__(self, name, d, scene_loader):
        import oracle

        build, o = RENDER_CASES[name] if name != RAY_CASE else (_cornell, {})
        self.name, self.path = name, build(d)
        register_textures(self.path)
        self.scene = scene_loader(self.path)
        self.W, self.H = o.get("size", (W, H))
        self.passes = o.get("passes", [])
        self.adaptive, self.min_samples, self.tolerance = bool(o.get("adaptive")), o.get("min_samples", 100), 0.05
        self.camera = np.asarray(self.scene.camera, np.float32).copy()
        if o.get("camera") == "h5":
            self.camera = hazards.h5_cameras(self.scene)[0]
        n = self.W * self.H
        if o.get("seeds") == "h7":
            self.seeds = hazards.h7_axis_seeds(self.W, self.H)
        elif o.get("seeds") == "h4":
            self.seeds, self.planted = hazards.h4_seeds(oracle.OracleScene(self.path), self.W, self.H)
        else:
            self.seeds = oracle.mt19937(n)

    def meta(self):
        return {"name": self.name, "width": self.W, "height": self.H, "passes": self.passes,
                "adaptive": self.adaptive, "min_samples": self.min_samples, "tolerance": self.tolerance,
                "planted": getattr(self, "planted", 0), "files": file_hashes(self.path)}

    def rays(self):
        """the hazard ray set of tests/test_gpu_query.py (on-split origins, NaN and infinite components,
        axis-parallel directions) and its in-box set, on this case's scene"""
        import test_gpu_query as q

        class _C:  # what make_rays asks of a test_gpu_query._Case for these classes
            osc = self.scene
            bounds = self.scene.arrays()[4].astype(np.float32)

        return np.concatenate([q.make_rays(_C, kind, n) for kind, n in RAY_KINDS]).astype(np.float32)


def run_frames(case, scene=None, counters=None):
    """the case's calls on `scene` (default: the case's own) -> the four G-buffer arrays after each call;
    `counters`: a dict that collects the oracle's counters (an OracleScene's render returns them)"""
    scene = scene or case.scene
    n = case.W * case.H
    fb, sq = np.zeros(n * 3, np.float32), np.zeros(n, np.float32)
    cnt, rng = np.zeros(n, np.int32), case.seeds.copy()
    out = []
    for c, passes in enumerate(case.passes):
        k = scene.render(case.camera, fb, sq, cnt, rng, case.W, case.H, passes, sample_count_arg=0 if c == 0 else 1,
                         adaptive=case.adaptive, min_samples=case.min_samples, tolerance=case.tolerance)
        if counters is not None and k:
            counters["maxdepth"] = max(counters.get("maxdepth", 0), k["maxdepth"])
            for key in ("deep_push", "watchdog", "cut"):
                counters[key] = counters.get(key, 0) + k[key]
            for key, v in k["hazards"].items():
                counters[key] = counters.get(key, 0) + v
        out.append((fb.reshape(n, 3).copy(), sq.copy(), cnt.copy(), rng.copy()))
    return out


def scene_bytes(scene):
    """a loaded scene's arrays (oracle.OracleScene, reference.ReferenceScene or ProductScene), comparable
    byte for byte: (triangles (n, 152) uint8, node bytes, indices, lights, bounds), the triangles' texel
    pointers (addresses) replaced by the first 8 bytes of a SHA-256 of the texels they point to"""
    import ctypes

    tb, nodes, idx, lights, bounds = scene.arrays()
    t = np.frombuffer(tb, np.uint8).reshape(-1, 152).copy()
    ptr = t[:, 136:144].copy().view(np.uint64)[:, 0]
    wh = t[:, 144:152].copy().view(np.int32)
    for k in np.nonzero(ptr)[0]:
        texels = ctypes.string_at(int(ptr[k]), int(wh[k, 0]) * int(wh[k, 1]) * 4)
        t[k, 136:144] = np.frombuffer(hashlib.sha256(texels).digest()[:8], np.uint8)
    return (t, bytes(nodes), np.ascontiguousarray(idx, np.int32), np.ascontiguousarray(lights, np.int32),
            np.ascontiguousarray(bounds, np.float32))


def scene_record(scene):
    """a loaded scene as the fixtures keep it: SHA-256 of scene_bytes' triangles, nodes and indices and
    their counts; the light list and the bounds themselves"""
    t, nodes, idx, lights, bounds = scene_bytes(scene)
    return {"triangles": hashlib.sha256(t.tobytes()).hexdigest(), "nodes": hashlib.sha256(nodes).hexdigest(),
            "indices": hashlib.sha256(idx.tobytes()).hexdigest(),
            "counts": [len(t), len(nodes) // 20, len(idx), len(lights)]}, lights, bounds


class ProductScene:
    """the product's host side (rt.HostScene: load_mesh; rt.build_kd_tree) with the arrays() of the other
    two.  The product builds its light list when it uploads a scene, so arrays() has none (lights: empty)."""

    def __init__(self, path):
        import rt

        self.host = rt.HostScene(path)
        self.camera = np.array(self.host.camera.as_list(), np.float32)

    def arrays(self):
        import rt

        tb, n = self.host.triangles_bytes()
        ptr, n = self.host.triangle_ptr()
        nodes, idx, bounds = rt.build_kd_tree(ptr, n)
        return tb, nodes, idx, np.zeros(0, np.int32), np.array(bounds, np.float32)


TONEMAP_CASE = "cornell"  # its fixture also holds the reference's display bytes of its final frame


def zeroed_counts(counts):
    """a non-finite case's final sample counts with every 7th set to 0 (the display divides by the count):
    its fixture holds the reference's display bytes of its final frame with these counts"""
    c = np.array(counts, np.int32)
    c[::7] = 0
    return c


def record(name, d):
    """(case, what a fixture holds for it), computed by the live reference (oracle/_ref/libref_rt.so)"""
    import reference

    case = Case(name, d, reference.ReferenceScene)
    meta = case.meta()
    meta["scene"], lights, bounds = scene_record(case.scene)
    out = {"camera": case.camera, "lights": lights.astype(np.int32), "bounds": bounds.astype(np.float32)}
    if name == RAY_CASE:
        out["rays"] = case.rays()
        out["samples"] = case.scene.trace_rays(out["rays"])  # the whole Sample, reference.SAMPLE_FIELDS
    else:
        out["seeds"] = case.seeds
        frames = run_frames(case)
        for c, arrays in enumerate(frames):
            for key, a in zip(G_NAMES, arrays):
                out[f"call{c}_{key}"] = a
        if name == TONEMAP_CASE:
            out["tonemap_rgba"] = reference.tonemap(frames[-1][0], frames[-1][2])
        if name in NONFINITE_CASES:
            out["tonemap_rgba"] = reference.tonemap(frames[-1][0], zeroed_counts(frames[-1][2]))
    out["meta"] = np.array(json.dumps(meta, sort_keys=True))
    return case, out


def fixture_frames(fx):
    """the recorded G-buffer arrays after each call"""
    return [tuple(fx[f"call{c}_{key}"] for key in G_NAMES) for c in range(len(fx["meta"]["passes"]))]


SAMPLE_ORACLE_COLUMNS = [0, 1] + list(range(12, 21))  # the reference's Sample columns that or_trace_rays reports


def same_bits(a, b):
    """equal bit for bit (float arrays: as uint32; NaNs of any payload equal each other, as
    test_independent._same), shapes included"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == np.float32:
        return bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))
    return bool(np.array_equal(a, b))


# ------------------------------------------------------------------ what a case's pixels meet first
def centre_rays(camera, W, H):
    """the camera's rays through the pixel centres (path_tracing()'s ray with both jitters 0.5, aperture 0), as
    (W * H, 6) float32 rows position, direction"""
    cam = np.asarray(camera, np.float32)
    cy, sy = np.float32(np.cos(np.float64(cam[3]))), np.float32(np.sin(np.float64(cam[3])))
    cp, sp = np.float32(np.cos(np.float64(cam[4]))), np.float32(np.sin(np.float64(cam[4])))
    R = (np.array([[cy, 0, -sy], [0, 1, 0], [sy, 0, cy]], np.float32).T  # rotation_matrix(yaw, pitch), roll 0:
         @ np.array([[1, 0, 0], [0, cp, sp], [0, -sp, cp]], np.float32).T)  # the reference lists columns
    t = np.float32(np.tan(np.float64(cam[5]) / 2))
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    d = np.stack([t * (x + 0.5 - W // 2) / (W // 2), t * (y + 0.5 - H // 2) / (W // 2), np.ones_like(x)], -1)
    d = (d / np.linalg.norm(d, axis=-1, keepdims=True)).reshape(-1, 3).astype(np.float32) @ R.T
    return np.concatenate([np.repeat(cam[None, :3], W * H, 0), d], axis=1).astype(np.float32)


def first_hits(case):
    """(rays, trace_rays' rows, material name or None) of the case's centre rays on the oracle; the name is read
    from the hit triangle's material, matched against the materials of the scene's .mat file"""
    import oracle

    osc = case.scene if isinstance(case.scene, oracle.OracleScene) else oracle.OracleScene(case.path)
    rays = centre_rays(case.camera, case.W, case.H)
    hits = osc.trace_rays(rays)
    tris = np.frombuffer(osc.arrays()[0], np.uint8).reshape(-1, 152)
    mat_file = [p for r, p in scene_input_files(case.path) if r.endswith(".mat")][0]
    names = [ln.split()[1] for ln in open(mat_file).read().splitlines() if ln.startswith("material ")]
    by_bytes = {}
    for nm in names:  # albedo, emittance, roughness, n, k, transparent: Triangle bytes 96..133
        rc_, m = oracle.load_material(mat_file, nm)
        assert rc_ == 1
        by_bytes[m.tobytes()] = nm
    out = []
    for h in hits:
        if h[0] != 1:
            out.append(None)
            continue
        t = tris[int(h[1])]
        key = np.concatenate([t[96:132].copy().view(np.float32), [np.float32(t[132])]]).astype(np.float32).tobytes()
        out.append(by_bytes[key])
    return rays, hits, out
