"""A numpy float32 restatement of rt_reproject's definition (DESIGN.md
"Temporal reprojection"; TEST INFRASTRUCTURE ONLY), written from the
definition and not from csrc/reproject_math.h, whole frames at a time — and
the synthetic frames the reprojection's tests share.

Every operation is a float32 numpy operation in the definition's order, so the
result has rt_reproject_host's and rt_reproject's bits.  The camera's frame
constants are the reference's: rotation_matrix (independent_path) with
correctly rounded cos / sin, tanf(FOV / 2) correctly rounded."""
import numpy as np

import independent_path as ip
import rt

F = np.float32
INF = F(np.inf)
DEFAULTS = dict(max_history=64, depth_tol=0.02, normal_min=0.95, match_triangle=True)
SNAP = F(1.0 / 64.0)
MIN_WEIGHT = F(1.0 / 16.0)


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def camera(pos, yaw=0.0, pitch=0.0, fov=1.2, aperture=0.0):
    return rt.Camera(rt.Vec3D(*[float(F(p)) for p in pos]), float(F(yaw)), float(F(pitch)), float(F(fov)),
                     float(F(aperture)))


def camera_constants(cam):
    """(R = (i, j, k) columns as float32 triples, tan(FOV / 2), position)"""
    with np.errstate(all="ignore"):
        R = ip.rotation_matrix(F(cam.yaw), F(cam.pitch))
        tan = np.tan(np.float64(F(cam.FOV) / F(2))).astype(F)
    return R, tan, (F(cam.position.x), F(cam.position.y), F(cam.position.z))


def centre_dirs(cam, W, H):
    """the pixel-centre directions of `cam`, three (H, W) float32 arrays (camera_ray with both draws 0.5)"""
    R, tan, _ = camera_constants(cam)
    ys, xs = np.mgrid[0:H, 0:W]
    hw, hh = F(W // 2), F(H // 2)
    with np.errstate(all="ignore"):
        px = tan * ((xs.astype(F) + F(0.5)) - hw) / hw
        py = tan * ((ys.astype(F) + F(0.5)) - hh) / hw
        pz = np.ones_like(px)
        r = F(1) / np.sqrt((px * px + py * py) + pz * pz)
        lx, ly, lz = px * r, py * r, pz * r
        return tuple((lx * R[0][c] + ly * R[1][c]) + lz * R[2][c] for c in range(3))


def _dot3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def reproject(src_fb, src_sq, src_count, aov_src, cam_src, aov_dst, cam_dst, max_history=0, depth_tol=0.0,
              normal_min=0.0, match_triangle=True):
    """-> (fb (H, W, 3) float32, sq (H, W) float32, count (H, W) int32, stats dict)"""
    max_history = max_history or DEFAULTS["max_history"]
    depth_tol = F(depth_tol or DEFAULTS["depth_tol"])
    normal_min = F(normal_min or DEFAULTS["normal_min"])
    z = np.asarray(aov_dst["depth"], F)
    H, W = z.shape
    s_fb = np.asarray(src_fb, F).reshape(H, W, 3)
    s_sq = np.asarray(src_sq, F).reshape(H, W)
    s_n = np.asarray(src_count, np.int32).reshape(H, W)
    s_z = np.asarray(aov_src["depth"], F).reshape(H, W)
    s_nrm = np.asarray(aov_src["normal"], F).reshape(H, W, 3)
    d_nrm = np.asarray(aov_dst["normal"], F).reshape(H, W, 3)
    s_tri, d_tri = aov_src.get("triangle"), aov_dst.get("triangle")
    match = bool(match_triangle) and s_tri is not None and d_tri is not None
    if match:
        s_tri, d_tri = np.asarray(s_tri, np.int32).reshape(H, W), np.asarray(d_tri, np.int32).reshape(H, W)
    Rs, tan_s, pos_s = camera_constants(cam_src)
    _, _, pos_d = camera_constants(cam_dst)
    hw, hh = F(W // 2), F(H // 2)
    with np.errstate(all="ignore"):
        alive = z < INF                                                         # 1
        d = centre_dirs(cam_dst, W, H)                                          # 2
        delta = tuple(pos_d[c] - pos_s[c] for c in range(3))
        v = tuple(delta[c] + d[c] * z for c in range(3))
        cx, cy, cz = _dot3(v, Rs[0]), _dot3(v, Rs[1]), _dot3(v, Rs[2])           # 3
        alive &= cz > F(0)
        u = ((cx / cz) / tan_s * hw + hw) - F(0.5)
        w = ((cy / cz) / tan_s * hw + hh) - F(0.5)
        alive &= (u > F(-1)) & (u < F(W)) & (w > F(-1)) & (w < F(H))
        u = np.where(alive, u, F(0))
        w = np.where(alive, w, F(0))
        z_exp = np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
        z_tol = depth_tol * z_exp
        ru, rw = np.floor(u + F(0.5)), np.floor(w + F(0.5))                     # 4
        snap = (np.abs(u - ru) <= SNAP) & (np.abs(w - rw) <= SNAP)
        fu, fw = np.floor(u), np.floor(w)
        ax, ay = u - fu, w - fw
        bx, by = F(1) - ax, F(1) - ay
        x0, y0 = fu.astype(np.int64), fw.astype(np.int64)
        one = np.ones_like(u)
        modes = {True: [(ru.astype(np.int64), rw.astype(np.int64), one)],
                 False: [(x0, y0, bx * by), (x0 + 1, y0, ax * by), (x0, y0 + 1, bx * ay), (x0 + 1, y0 + 1, ax * ay)]}
        results = {}
        for is_snap, taps in modes.items():
            wsum = np.zeros((H, W), F)
            n_h = np.full((H, W), 0x7FFFFFFF, np.int64)
            m = [np.zeros((H, W), F) for _ in range(4)]
            first_n = None
            first_q = None
            for tx, ty, tw in taps:                                             # 5
                ok = (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)
                qx, qy = np.clip(tx, 0, W - 1), np.clip(ty, 0, H - 1)
                n = s_n[qy, qx].astype(np.int64)
                zq = s_z[qy, qx]
                ok &= (n > 0) & (zq < INF) & (np.abs(zq - z_exp) <= z_tol)
                nq = s_nrm[qy, qx]
                ok &= _dot3((d_nrm[..., 0], d_nrm[..., 1], d_nrm[..., 2]), (nq[..., 0], nq[..., 1], nq[..., 2])) >= normal_min
                if match:
                    ok &= s_tri[qy, qx] == d_tri
                wsum = np.where(ok, wsum + tw, wsum)                            # 6
                n_h = np.where(ok & (n < n_h), n, n_h)
                fn = np.where(n > 0, n, 1).astype(F)
                inv = F(1) / fn
                f = s_fb[qy, qx]
                for c in range(3):
                    m[c] = np.where(ok, m[c] + tw * (f[..., c] * inv), m[c])
                m[3] = np.where(ok, m[3] + tw * (s_sq[qy, qx] / fn), m[3])
                if first_n is None:
                    first_n, first_q = np.where(ok, n, 0), (qy, qx)
            keep = wsum >= MIN_WEIGHT
            n_h = np.minimum(n_h, max_history)
            nf = n_h.astype(F)
            out_fb = np.stack([m[c] / wsum * nf for c in range(3)], axis=-1)     # 7
            out_sq = m[3] / wsum * nf
            if is_snap:
                exact = keep & (n_h == first_n)
                out_fb = np.where(exact[..., None], s_fb[first_q], out_fb)
                out_sq = np.where(exact, s_sq[first_q], out_sq)
            results[is_snap] = (keep, out_fb, out_sq, n_h)
        keep = alive & np.where(snap, results[True][0], results[False][0])
        fb = np.where(snap[..., None], results[True][1], results[False][1])
        sq = np.where(snap, results[True][2], results[False][2])
        cnt = np.where(snap, results[True][3], results[False][3])
        keep &= np.isfinite(fb).all(axis=-1) & np.isfinite(sq)  # a non-finite sum is not carried
    fb = np.where(keep[..., None], fb, F(0)).astype(F)
    sq = np.where(keep, sq, F(0)).astype(F)
    cnt = np.where(keep, cnt, 0).astype(np.int32)
    stats = dict(pixels=W * H, kept_pixels=int((cnt > 0).sum()), carried_samples=int(cnt.astype(np.int64).sum()))
    return fb, sq, cnt, stats


# ---------------------------------------------------------------- synthetic frames
# An analytic room for guides that agree between two cameras: a floor, a back wall, a free-standing panel in
# front of it (disocclusions when the camera moves) and open sky above (misses).  Each surface is cut into
# unit squares with ids of their own, so triangle matching has edges to find.
_SURFACES = [  # (axis, offset, normal, bounds of the other two axes in x, y, z order, id base)
    (1, 0.0, (0.0, 1.0, 0.0), ((-30.0, 30.0), None, (-30.0, 10.0)), 1000),
    (2, 10.0, (0.0, 0.0, -1.0), ((-30.0, 30.0), (0.0, 5.0), None), 2000),
    (2, 4.0, (0.0, 0.0, -1.0), ((-0.6, 0.7), (0.0, 2.2), None), 3000),
]


def cast(cam, W, H):
    """first-hit AOVs of the analytic room: depth (H, W) float32 (inf: miss), normal (H, W, 3), triangle (H, W)"""
    d = np.stack(centre_dirs(cam, W, H), axis=-1).astype(np.float64)
    o = np.array([cam.position.x, cam.position.y, cam.position.z], np.float64)
    best = np.full((H, W), np.inf)
    normal = np.zeros((H, W, 3), F)
    tri = np.full((H, W), -1, np.int32)
    with np.errstate(all="ignore"):
        for axis, off, nrm, bounds, base in _SURFACES:
            t = (off - o[axis]) / d[..., axis]
            p = o + d * t[..., None]
            ok = (t > 1e-4) & (t < best)
            for a in range(3):
                if bounds[a] is not None:
                    ok &= (p[..., a] >= bounds[a][0]) & (p[..., a] <= bounds[a][1])
            cell = np.floor(p).astype(np.int64)
            other = [a for a in range(3) if a != axis]
            ids = base + (cell[..., other[0]] % 64) * 64 + (cell[..., other[1]] % 64)
            best = np.where(ok, t, best)
            normal = np.where(ok[..., None], np.asarray(nrm, F), normal)
            tri = np.where(ok, ids, tri).astype(np.int32)
    return dict(depth=best.astype(F), normal=normal, triangle=tri)


def sums(W, H, seed, counts=(0, 1, 2, 7, 20, 64, 300)):
    """random per-pixel sums with the given sample counts mixed"""
    rs = np.random.RandomState(seed)
    count = rs.choice(np.asarray(counts, np.int32), size=(H, W)).astype(np.int32)
    mean = rs.uniform(0.0, 3.0, size=(H, W, 3)).astype(F)
    fb = (mean * count[..., None].astype(F)).astype(F)
    sq = (rs.uniform(0.0, 9.0, size=(H, W)).astype(F) * count.astype(F)).astype(F)
    return fb, sq, count


CAM_A = dict(pos=(0.3, 1.5, -2.0), yaw=0.1, pitch=-0.05, fov=1.2)
SHAPES = [(64, 48), (67, 45), (1, 1)]
CASES = ["unmoved", "small_move", "dolly_in", "large_turn", "behind", "far_unmoved", "no_triangles", "tight_options",
         "nan_depth", "nan_camera", "inf_camera", "nan_src_camera", "nan_sums"]


def case(name, W, H):
    """-> (src sums (fb, sq, count), aov_src, cam_src, aov_dst, cam_dst, options)"""
    opts = {}
    a = camera(**CAM_A)
    b = a
    if name == "small_move":
        b = camera((0.55, 1.45, -1.8), 0.15, -0.05, 1.2)
    elif name == "dolly_in":
        b = camera((0.3, 1.5, 0.5), 0.1, -0.05, 1.2)
    elif name == "large_turn":
        b = camera(CAM_A["pos"], 0.1 + np.pi, -0.05, 1.2)
    elif name == "behind":  # the new camera stands well behind the old one: much of what it sees is behind that
        a = camera((0.3, 1.5, 6.0), 0.1, -0.05, 1.2)
        b = camera((0.3, 1.5, -2.0), 0.1, -0.05, 1.2)
    elif name == "tight_options":
        b = camera((0.4, 1.5, -1.9), 0.12, -0.06, 1.2)
        opts = dict(max_history=16, depth_tol=0.001, normal_min=0.999, match_triangle=False)
    elif name == "no_triangles":
        b = camera((0.4, 1.5, -1.9), 0.12, -0.06, 1.2)
    elif name == "nan_camera":
        b = camera((float("nan"), 1.5, -2.0), 0.1, -0.05, 1.2)
    elif name == "inf_camera":
        b = camera((0.3, float("inf"), -2.0), float("inf"), -0.05, 1.2)
    src = sums(W, H, 7)
    if name == "nan_sums":  # fireflies gone wrong in the old frame: NaN and Inf sums, after a move and in place
        b = camera((0.4, 1.5, -1.9), 0.12, -0.06, 1.2) if W % 2 else a
        rs = np.random.RandomState(17)
        r = rs.uniform(size=(H, W))
        src[0][r < 0.05, 1] = F(np.nan)
        src[0][(r >= 0.05) & (r < 0.1), 2] = INF
        src[1][(r >= 0.1) & (r < 0.15)] = F(np.nan)
    if name == "far_unmoved":  # |position| ~ 50, depths 0.01 .. 1000 that no geometry made
        a = b = camera((31.0, -22.5, 33.0), 2.3, 0.4, 0.9)
        rs = np.random.RandomState(11)
        depth = np.exp(rs.uniform(np.log(0.01), np.log(1000.0), size=(H, W))).astype(F)
        depth[rs.uniform(size=(H, W)) < 0.1] = INF
        nrm = rs.normal(size=(H, W, 3))
        nrm = (nrm / np.linalg.norm(nrm, axis=-1, keepdims=True)).astype(F)
        aov = dict(depth=depth, normal=nrm, triangle=rs.randint(0, 50, size=(H, W)).astype(np.int32))
        return src, aov, a, dict(aov), b, opts
    aov_a, aov_b = cast(a, W, H), cast(b, W, H)
    if name == "nan_src_camera":  # (the guides are the good camera's: only the projection sees the NaN)
        a = camera((0.3, 1.5, -2.0), float("nan"), -0.05, 1.2)
    if name == "no_triangles":
        aov_a.pop("triangle")
    if name == "nan_depth":
        rs = np.random.RandomState(13)
        r = rs.uniform(size=(H, W))
        aov_b["depth"] = np.where(r < 0.2, F(np.nan), np.where(r < 0.4, -INF, np.where(r < 0.5, F(-3.0), aov_b["depth"])))
        aov_b["depth"] = aov_b["depth"].astype(F)
    return src, aov_a, a, aov_b, b, opts


def plane_case(W, H, dist, shift_x=0.0, shift_y=0.0, counts=None, seed=5):
    """a plane at `dist` perpendicular to the view axis (yaw = pitch = 0), seen before and after a sideways
    move of (shift_x, shift_y) pixels: depths are the radial dist * |pixel direction|"""
    fov = 1.2
    a = camera((0.25, -0.5, 1.0), 0.0, 0.0, fov)
    _, tan, pos = camera_constants(a)
    step = F(dist) * tan / F(W // 2)  # one pixel on the plane
    b = camera((pos[0] + F(shift_x) * step, pos[1] + F(shift_y) * step, pos[2]), 0.0, 0.0, fov)
    ys, xs = np.mgrid[0:H, 0:W]
    px = np.float64(tan) * (xs + 0.5 - W // 2) / (W // 2)
    py = np.float64(tan) * (ys + 0.5 - H // 2) / (W // 2)
    depth = (dist * np.sqrt(px * px + py * py + 1.0)).astype(F)
    nrm = np.zeros((H, W, 3), F)
    nrm[..., 2] = -1
    aov = dict(depth=depth, normal=nrm, triangle=np.full((H, W), 5, np.int32))
    fb, sq, count = sums(W, H, seed, counts=(1, 2, 7, 20, 64))
    if counts is not None:
        mean = fb / count[..., None].astype(F)
        count = np.broadcast_to(np.asarray(counts, np.int32), (H, W)).copy()
        fb = (mean * count[..., None].astype(F)).astype(F)
    return (fb, sq, count), aov, a, {k: v.copy() for k, v in aov.items()}, b
