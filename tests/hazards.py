"""Inputs built to trigger the reference's numerical hazards (SURVEY
Appendix A) — test helpers for tests/test_gpu_hazards.py and
tests/test_hazards_cpu.py.

The per-pixel RNG of the reference (get_random_unilateral,
rt/path_tracing.cuh:34-43) is x' = out(x * 747796405 + 2891336453) with the
PCG RXS-M-XS output permutation out(s) = w ^ (w >> 22),
w = ((s >> ((s >> 28) + 4)) ^ s) * 277803737.  Every step is a bijection
of the 32-bit words, so the G-buffer seed that makes the k-th draw of a pass
return a chosen word can be computed backwards (rng_back).
"""
import os

import numpy as np

M_LCG, C_LCG, M_OUT = 747796405, 2891336453, 277803737
MASK = 0xFFFFFFFF


def rng_step(x):
    """one draw: the new state (= the returned word)"""
    s = (x * M_LCG + C_LCG) & MASK
    w = (((s >> ((s >> 28) + 4)) ^ s) * M_OUT) & MASK
    return (w >> 22) ^ w


def rng_step_inv(r):
    """the state x with rng_step(x) == r"""
    w = r ^ (r >> 22)  # bits 31..22 of w and r agree
    s_xs = (w * pow(M_OUT, -1, 1 << 32)) & MASK
    s = s_xs  # invert s ^ (s >> k): the top 4 bits fix k = (s >> 28) + 4 >= 4
    k = (s_xs >> 28) + 4
    for _ in range(8):
        s = s_xs ^ (s >> k)
    return ((s - C_LCG) * pow(M_LCG, -1, 1 << 32)) & MASK


def rng_back(word, k):
    """the seed whose (k+1)-th draw (index k) returns `word`"""
    x = word
    for _ in range(k + 1):
        x = rng_step_inv(x)
    return x


def unilateral(word):
    """the float the reference returns for a drawn word: float(x) / UINT32_MAX in f32"""
    return np.float32(np.float32(word) / np.float32(4294967295.0))


# words whose draw is exactly 1.0f: float(x) rounds to 2^32
ONE_WORDS = range((1 << 32) - 128, 1 << 32)


def cornell_variant(d, name, yaw_room=0.1, camera=None, extra_obj="", extra_mat=""):
    """The cornell scene's geometry (build/scenes/cornell) with the room
    rotated by `yaw_room` (0: every wall axis-aligned, so KD split planes
    coincide with wall planes) and an optional camera line / extra faces."""
    import helpers

    src = os.path.dirname(helpers.scene_path("cornell"))
    os.makedirs(d, exist_ok=True)
    obj = open(os.path.join(src, "cornell.obj")).read() + extra_obj
    mat = open(os.path.join(src, "cornell.mat")).read() + extra_mat
    with open(os.path.join(d, f"{name}.obj"), "w") as f:
        f.write(obj)
    with open(os.path.join(d, f"{name}.mat"), "w") as f:
        f.write(mat)
    cam = camera or "-0.3458 1.0 -3.5834 0.1 0 0.8 0"
    p = os.path.join(d, "scene.txt")
    with open(p, "w") as f:
        f.write(f"mesh {name}.obj {name}.mat 0 1 0 {yaw_room} 0 1 0\ncamera {cam}\n")
    return p


def root_split(osc):
    """(axis, offset) of the KD root (20-B reference nodes: plane_axis u8 @8, plane_offset f32 @12)"""
    _, nodes, _, _, _ = osc.arrays()
    axis = nodes[8]
    off = np.frombuffer(nodes[12:16], dtype=np.float32)[0]
    return int(axis), np.float32(off)


# ------------------------------------------------------------ input builders
def h4_seeds(osc, W, H, step=5, k=9):
    """mt19937 seeds with every `step`-th pixel replaced by a seed whose draw
    k (the NEE light pick of a pass whose first bounce is diffuse) returns a
    word whose float is exactly 1.0 — kept only where the oracle confirms the
    pick happened (single-pixel oracle runs).  Returns (seeds, planted)."""
    n = W * H
    rng0 = _mt(n)
    planted = 0
    for pix in range(0, n, step):
        for word in ONE_WORDS:
            seed = rng_back(word, k)
            trial = rng0.copy()
            trial[pix] = seed  # (the render advances trial in place)
            fb, sq, ct = np.zeros(n * 3, np.float32), np.zeros(n, np.float32), np.zeros(n, np.int32)
            c = osc.render(osc.camera, fb, sq, ct, trial, W, H, 1, sample_count_arg=0,
                           pixels=np.array([pix], np.int32), adaptive=False)
            if c["hazards"]["xi_one"]:
                rng0[pix] = seed
                planted += 1
                break
    return rng0, planted


def h5_cameras(osc):
    """(camera on the root split plane, camera one ulp off it), aperture 0"""
    axis, split = root_split(osc)
    on = osc.camera.copy()
    on[6] = 0.0
    on[axis] = split
    off = on.copy()
    off[axis] = np.nextafter(split, np.float32(np.inf))
    return on, off


def h7_axis_seeds(W, H):
    """seeds: column x = W/2 - 1 draws 1.0f first (x jitter: direction.x ==
    0 for an axis-aligned camera), row y = H/2 - 1 draws 1.0f second
    (direction.y == 0)"""
    rng0 = _mt(W * H)
    one = (1 << 32) - 1
    for y in range(H):
        rng0[y * W + W // 2 - 1] = rng_back(one, 0)
    for x in range(W):
        rng0[(H // 2 - 1) * W + x] = rng_back(one, 1)
    return rng0


AXIS_CAMERA = "-0.3458 1.0 -3.5834 0 0 0.8 0"  # yaw 0, pitch 0, aperture 0: rotation = identity exactly

# zero-area triangles in the middle of the room: a repeated vertex (cross
# product exactly 0 after any transform: normalize -> NaN), three collinear
# points, and a nearly collinear one
DEGENERATE_OBJ = ("\nusemtl white\nv 0.2 1.2 0.3\nv 0.2 1.2 0.3\nv -0.1 0.9 0.2\nf -3 -2 -1\n"
                  "v -0.5 0.5 0.1\nv 0.0 0.5 0.1\nv 0.5 0.5 0.1\nf -3 -2 -1\n"
                  "v -0.4 0.3 -0.2\nv 0.4 1.3 0.4\nv 0.0 0.8 0.1\nf -3 -2 -1\n"
                  "v 0.1 0.2 -0.3\nv 0.1 1.6 -0.3\nv 0.1 1.6 -0.3\nf -3 -2 -1\n")


# The same two triangles twice, red then green, facing the camera: every hit on
# the quad has two passing tests at exactly the same s (identical records), the
# reference keeps the first listed in its leaf (strict <), and the bounded
# traversal's T* leaf shortcut must step aside (bvh_trace.h leaf_scan_min: a
# tie) — the colour says which copy won.
DUPLICATE_OBJ = ("\nusemtl red\nv -0.45 0.35 0.25\nv 0.45 0.35 0.25\nv 0.45 1.25 0.25\nv -0.45 1.25 0.25\n"
                 "f -4 -3 -2\nf -4 -2 -1\n"
                 "usemtl green\nv -0.45 0.35 0.25\nv 0.45 0.35 0.25\nv 0.45 1.25 0.25\nv -0.45 1.25 0.25\n"
                 "f -4 -3 -2\nf -4 -2 -1\n")

def _mt(n):
    import oracle

    return oracle.mt19937(n)


# ------------------------------------------------------------ adversarial geometry
ADV_MAT = ("material white\nalbedo 0.73 0.73 0.73\nroughness 0.5\nn 1.5\n\n"
           "material red\nalbedo 0.65 0.05 0.05\nroughness 0.5\nn 1.5\n\n"
           "material gold\nalbedo 0.9 0.7 0.3\nroughness 0.15\nn 1.2\nk 3.0\n\n"
           "material glass\nalbedo 0.99 0.99 0.99\nroughness 0.01\nn 1.5\ntransparent\n\n"
           "material light\nalbedo 0.78 0.78 0.78\nemittance 15.0 15.0 15.0\nroughness 0.5\nn 1.5\n")


def _adversarial_obj(seed):
    """A closed room (y in [0, 2]) holding the cases the BVH margins are
    hardest on: slivers (a vertex 1e-7..1e-2 of the edge length off the
    opposite edge), needles (two vertices 1e-7..1e-3 apart), near-degenerate
    fans sharing a vertex, and a dense cluster of tiny triangles — in every
    orientation, some axis-aligned."""
    rng = np.random.default_rng(seed)
    lines = ["# adversarial room"]
    vs = []

    def quad(mat, a, b, c, d):
        base = len(vs) + 1
        vs.extend([a, b, c, d])
        lines.append(f"usemtl {mat}")
        lines.append(f"f {base} {base + 1} {base + 2} {base + 3}")

    def tri(mat, a, b, c):
        base = len(vs) + 1
        vs.extend([a, b, c])
        lines.append(f"usemtl {mat}")
        lines.append(f"f {base} {base + 1} {base + 2}")

    quad("white", (-1, 0, -1), (1, 0, -1), (1, 0, 1), (-1, 0, 1))
    quad("white", (-1, 2, -1), (-1, 2, 1), (1, 2, 1), (1, 2, -1))
    quad("white", (-1, 0, 1), (1, 0, 1), (1, 2, 1), (-1, 2, 1))
    quad("red", (-1, 0, -1), (-1, 0, 1), (-1, 2, 1), (-1, 2, -1))
    quad("white", (1, 0, -1), (1, 2, -1), (1, 2, 1), (1, 0, 1))
    quad("light", (-0.3, 1.98, -0.3), (0.3, 1.98, -0.3), (0.3, 1.98, 0.3), (-0.3, 1.98, 0.3))

    def unit():
        v = rng.normal(size=3)
        return v / np.linalg.norm(v)

    mats = ["white", "gold", "glass", "red"]
    for k in range(300):  # slivers
        c = rng.uniform([-0.8, 0.2, -0.8], [0.8, 1.8, 0.8])
        u, w = unit(), unit()
        if k % 5 == 0:  # axis-aligned edge and offset
            u, w = np.eye(3)[k % 3], np.eye(3)[(k + 1) % 3]
        L = 10 ** rng.uniform(-2.5, -0.5)
        eps = L * 10 ** rng.uniform(-7, -2)
        p1, p2 = c, c + L * u
        p3 = c + L * rng.uniform(0, 1) * u + eps * w
        tri(mats[k % 4], p1, p2, p3)
    for k in range(300):  # needles
        c = rng.uniform([-0.8, 0.2, -0.8], [0.8, 1.8, 0.8])
        u, w = unit(), unit()
        L = 10 ** rng.uniform(-2, -0.3)
        p2 = c + L * u
        tri(mats[(k + 1) % 4], c, p2, p2 + L * 10 ** rng.uniform(-7, -3) * w)
    for k in range(20):  # fans of thin wedges around a shared vertex
        c = rng.uniform([-0.6, 0.4, -0.6], [0.6, 1.6, 0.6])
        u, w = unit(), unit()
        w = w - np.dot(w, u) * u
        w /= np.linalg.norm(w)
        L = 10 ** rng.uniform(-1.5, -0.7)
        angs = np.sort(rng.uniform(0, 2 * np.pi, 24))
        for a0, a1 in zip(angs[:-1], angs[1:]):
            tri(mats[k % 4], c, c + L * (np.cos(a0) * u + np.sin(a0) * w), c + L * (np.cos(a1) * u + np.sin(a1) * w))
    cl = np.array([0.2, 0.9, 0.1])  # a cloud of tiny triangles (1e-4..1e-3 of the room)
    for k in range(400):
        c = cl + rng.normal(scale=0.05, size=3)
        s = 2 * 10 ** rng.uniform(-4, -3)
        tri(mats[k % 3], c, c + s * unit(), c + s * unit())
    out = [lines[0]] + [f"v {x:.9g} {y:.9g} {z:.9g}" for x, y, z in vs] + lines[1:]
    return "\n".join(out) + "\n"


def adversarial_scene(d, variant="far", seed=1):
    """The adversarial room (_adversarial_obj) placed where float rounding is
    coarsest relative to its features:
      far   — translated to x = 1.2e4, z = -8e3 (|x| ~ 10^4, 1 ulp ~ 1e-3 m);
      tiny  — scaled to 2 cm and placed 100 units from the origin, so its
              cloud triangles are sub-millimetre (0.2-2 um .. 20 um) 100 m away;
      near  — at the origin (reference)."""
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "adv.obj"), "w") as f:
        f.write(_adversarial_obj(seed))
    with open(os.path.join(d, "adv.mat"), "w") as f:
        f.write(ADV_MAT)
    ox, oy, oz, sc = {"far": (12000.0, 1.0, -8000.0, 1.0), "tiny": (100.0, 0.01, 0.0, 0.01),
                      "near": (0.0, 1.0, 0.0, 1.0)}[variant]
    cam = (ox - 0.3458 * sc, oy, oz - 3.5834 * sc)
    p = os.path.join(d, "scene.txt")
    with open(p, "w") as f:
        f.write(f"mesh adv.obj adv.mat {ox!r} {oy!r} {oz!r} 0.1 0 {sc!r} 0\n"
                f"camera {cam[0]!r} {cam[1]!r} {cam[2]!r} 0.1 0 0.8 0.0001\n")
    return p


# ------------------------------------------------------------ the material space
# One box per material: the BSDF's extremes, which no rendered scene reaches otherwise.  Every number is written
# as a literal that strtof parses to a normal f32 (the reference's std::stof throws on a denormal result); the
# denormals arise in the arithmetic: roughness and k of 1e-20 square to 1e-40, an albedo of 1e-21 gives a squared
# luminance of about 1e-41.
def _mat(albedo="0.8 0.8 0.8", roughness="0.1", n="1.5", k=None, transparent=False, emittance=None, texture=None):
    t = f"albedo {albedo}\n"
    if emittance:
        t += f"emittance {emittance}\n"
    t += f"roughness {roughness}\nn {n}\n"
    if k:
        t += f"k {k}\n"
    if transparent:
        t += "transparent\n"
    if texture:
        t += f"texture {texture}\n"
    return t


MATERIALS_TEXTURE = ("textures/box.png", "png_pal8_trns")  # (path in the .mat file, texture_fixtures variant)
ROOM_MATERIALS = {"wall": _mat("0.75 0.75 0.75", "0.5"), "floor": _mat("0.97 0.97 0.97", "0.5"),
                  "lamp": _mat("0 0 0", "0.5", emittance="4.0 4.0 4.0")}  # the lamp ends every path that meets it


def material_set():
    """name -> .mat text of the `materials` scene's boxes"""
    m = {}
    for r in ("0", "1e-20", "1e-4", "0.05", "0.5", "1", "1.5"):
        m[f"rough_{r}_dielectric"] = _mat("0.7 0.6 0.5", r)
        m[f"rough_{r}_glass"] = _mat("0.97 0.97 0.97", r, transparent=True)
        m[f"rough_{r}_conductor"] = _mat("0.9 0.7 0.3", r, n="1.2", k="3.0")
    for n in ("1.0", "1.0001", "4", "0.5", "100"):  # 0.5 in the middle of the grid: it transmits within 30 degrees
        m[f"n_{n}_opaque"] = _mat("0.6 0.7 0.8", n=n)
        m[f"n_{n}_transparent"] = _mat("0.97 0.97 0.97", n=n, transparent=True)
    for k in ("1e-20", "1e-3", "0.25", "50"):
        m[f"k_{k}"] = _mat("0.9 0.8 0.7", n="1.2", k=k)
    m["albedo_0_opaque"] = _mat("0 0 0")
    m["albedo_0_transparent"] = _mat("0 0 0", transparent=True)
    m["albedo_2"] = _mat("2.0 2.0 2.0", "0.5")
    m["albedo_1e-30"] = _mat("1e-30 1e-30 1e-30", "0.5")
    m["albedo_1e-21"] = _mat("1e-21 1e-21 1e-21", "0.5")  # squared luminance about 1e-41
    m["emissive_glass"] = _mat("0.97 0.97 0.97", "0.05", transparent=True, emittance="2.0 1.5 1.0")
    m["emissive_metal"] = _mat("0.9 0.7 0.3", "0.2", n="1.2", k="3.0", emittance="1.0 1.5 2.0")
    m["dim_emitter"] = _mat("0.5 0.5 0.5", "0.5", emittance="1e-9 1e-9 1e-9")  # NEE from it onto albedo 1e-30
    m["guide_n_4"] = _mat("0.999 0.999 0.999", "0.001", n="4", transparent=True)  # smooth and clear: deep paths
    m["guide_n_100"] = _mat("0.999 0.999 0.999", "0.001", n="100", transparent=True)
    m["textured"] = _mat("0.9 0.85 0.8", "0.4", texture=MATERIALS_TEXTURE[0])
    return m


def nonfinite_material_set():
    """the boxes of `materials_nonfinite`: three ordinary materials and the values that make NaN and Inf.  3e38
    and 1e30 are finite f32 numbers: the overflow happens in the products (3e38 * 3e38, 1e30 * 1e30)"""
    m = {"plain": _mat("0.7 0.6 0.5", "0.5"), "glass": _mat("0.97 0.97 0.97", "0.01", transparent=True),
         "gold": _mat("0.9 0.7 0.3", "0.15", n="1.2", k="3.0"),
         "emittance_3e38": _mat("0.5 0.5 0.5", "0.5", emittance="3e38 3e38 3e38"),
         "albedo_3e38_diffuse": _mat("3e38 3e38 3e38", "0.5"),
         "albedo_3e38_glass": _mat("3e38 3e38 3e38", "0.05", transparent=True),
         "albedo_3e38_metal": _mat("3e38 3e38 3e38", "0.15", n="1.2", k="3.0"),
         "rough_1e30": _mat("0.7 0.6 0.5", "1e30"),
         "n_1e30": _mat("0.7 0.6 0.5", n="1e30"),
         "n_0_opaque": _mat("0.7 0.6 0.5", n="0"),
         "n_0_transparent": _mat("0.97 0.97 0.97", n="0", transparent=True),
         "k_1e30": _mat("0.9 0.7 0.3", n="1.2", k="1e30")}
    return m


MATERIALS_GRID = (8, 6)  # boxes across x and z: the frame's 4:3
# Just under the lamp ceiling, looking straight down at the whole grid, so that what a box top reflects meets
# the lamp.  Off the symmetry planes, where the KD splits lie: a ray origin on a split plane is a hazard of its
# own (H5).
MATERIALS_CAMERA = "0.013 2.4 0.007 0 1.5707964 2.161 0"


def materials_scene(d, mats=None, name="materials"):
    """A room with a floor, four walls and, above a gap, a lamp ceiling; on the floor a grid of small boxes, one
    material per box in the order of `mats` (default material_set(); the cells beyond the set repeat its first
    three).  A box is a top and four sides, and the floor closes it, so a transparent one is entered and left.
    The room is open at the gap between the walls and the lamp: a path whose throughput has become NaN survives
    every roulette and ends only when it leaves the scene.  The camera looks straight down from under the lamp,
    so every box top is met close to its normal.  Returns the scene file."""
    import texture_fixtures

    mats = mats or material_set()
    os.makedirs(os.path.join(d, "textures"), exist_ok=True)
    if any(MATERIALS_TEXTURE[0] in t for t in mats.values()):
        with open(os.path.join(d, MATERIALS_TEXTURE[0]), "wb") as f:
            f.write(texture_fixtures.variants()[MATERIALS_TEXTURE[1]])
    with open(os.path.join(d, f"{name}.mat"), "w") as f:
        f.write("\n".join(f"material {k}\n{t}" for k, t in {**ROOM_MATERIALS, **mats}.items()))
    nx, nz = MATERIALS_GRID
    X, Z, Y = nx / 2 + 0.5, nz / 2 + 0.5, 1.5
    vs, faces = [], []

    def quad(mat, a, b, c, e, uv=False):
        base = len(vs) + 1
        vs.extend([a, b, c, e])
        faces.append(f"usemtl {mat}")
        faces.append("f " + " ".join(f"{base + j}/{j + 1}" if uv else f"{base + j}" for j in range(4)))

    quad("floor", (-X, 0, -Z), (X, 0, -Z), (X, 0, Z), (-X, 0, Z))
    quad("wall", (-X, 0, Z), (X, 0, Z), (X, Y, Z), (-X, Y, Z))
    quad("wall", (-X, 0, -Z), (-X, Y, -Z), (X, Y, -Z), (X, 0, -Z))
    quad("wall", (X, 0, -Z), (X, Y, -Z), (X, Y, Z), (X, 0, Z))
    quad("wall", (-X, 0, -Z), (-X, 0, Z), (-X, Y, Z), (-X, Y, -Z))
    for k in range(36):  # the lamp: a ceiling of strips above the walls (in strips, because the light pick is
        x0 = -X + 0.25 * k  # uniform over emissive triangles, boxes included)
        quad("lamp", (x0, 2.5, -Z), (x0 + 0.25, 2.5, -Z), (x0 + 0.25, 2.5, Z), (x0, 2.5, Z))
    names = list(mats)
    for cell in range(nx * nz):
        mat = names[cell] if cell < len(names) else names[cell % 3]
        cx, cz = cell % nx - nx / 2 + 0.5, cell // nx - nz / 2 + 0.5
        x0, x1, z0, z1, h = cx - 0.4, cx + 0.4, cz - 0.4, cz + 0.4, 0.4
        uv = "texture" in mats[mat]
        quad(mat, (x0, h, z0), (x0, h, z1), (x1, h, z1), (x1, h, z0), uv)
        quad(mat, (x0, 0, z0), (x0, h, z0), (x1, h, z0), (x1, 0, z0), uv)
        quad(mat, (x0, 0, z1), (x1, 0, z1), (x1, h, z1), (x0, h, z1), uv)
        quad(mat, (x0, 0, z0), (x0, 0, z1), (x0, h, z1), (x0, h, z0), uv)
        quad(mat, (x1, 0, z0), (x1, h, z0), (x1, h, z1), (x1, 0, z1), uv)
    vt = [(-0.3, -0.2), (1.7, -0.2), (1.7, 1.4), (-0.3, 1.4)]  # past [0, 1]: the mod wrap
    with open(os.path.join(d, f"{name}.obj"), "w") as f:
        f.write("\n".join([f"v {x} {y} {z}" for x, y, z in vs] + [f"vt {a} {b}" for a, b in vt] + faces) + "\n")
    p = os.path.join(d, "scene.txt")
    lo, hi = np.min(vs, axis=0), np.max(vs, axis=0)
    with open(p, "w") as f:  # the loader re-centres a mesh on its offset: the mesh's own centre keeps it in place
        f.write(f"mesh {name}.obj {name}.mat 0 {(lo[1] + hi[1]) / 2} 0 0 0 1 0\ncamera {MATERIALS_CAMERA}\n")
    return p


def materials_nonfinite_scene(d):
    return materials_scene(d, nonfinite_material_set(), "materials_nonfinite")
