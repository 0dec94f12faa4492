"""Frames the tests of rt_sample_aov / rt_denoise_sampler / rt_reproject_sampler share (TEST INFRASTRUCTURE
ONLY): samplers of the four image kinds and synthetic guides that are consistent between two cameras without a
scene — a sphere of per-pixel depths around an unmoved or yawed camera, a fronto-parallel plane under an
orthographic one.  Everything is seeded and built once per key; the arrays are read-only."""
import numpy as np

import reproject_ref as rref
import rt

F = np.float32
INF = F(np.inf)
PI = F(3.1415926536)
TAU = F(PI * F(2))
KINDS = ("pinhole", "equirect", "fisheye", "ortho")
bits = rref.bits

CAM_PLAIN = dict(pos=(0.25, -0.5, 1.0), yaw=0.0, pitch=0.0)
CAM_ROTATED = dict(pos=(31.0, -22.5, 33.0), yaw=2.3, pitch=0.4)


def sampler(kind, W, H, pos=(0.0, 0.0, 0.0), yaw=0.0, pitch=0.0, fov=None, ortho_half_width=2.0, pixels=None):
    """an rt.Sampler of an image kind; fov None: 1.2 for pinhole, 3.0 for fisheye"""
    if fov is None:
        fov = 3.0 if kind == "fisheye" else 1.2
    return rt.Sampler(kind, W, H, rref.camera(pos, yaw, pitch, fov), ortho_half_width=ortho_half_width, pixels=pixels)


def in_frame(smp):
    """(H, W) bool: the pixels that have a centre ray (all but a fisheye's pixels outside the image circle)"""
    rays = rt.sampler_rays_host(smp)
    return (rays[:, 3:] != 0).any(axis=1).reshape(smp.height, smp.width)


def guides(smp, seed, depth=None, miss_fraction=0.1, blocks=False):
    """synthetic first-hit AOVs for `smp`: a depth per pixel (`depth`, or log-uniform in 0.37 .. 55), unit normals,
    triangle ids (blocks: three normals in bands of 16 columns, ids in 8 x 8 blocks; else a normal and an id of
    its own per pixel); a tenth of the pixels and every pixel without a centre ray miss"""
    H, W = smp.height, smp.width
    rs = np.random.RandomState(seed)
    z = np.exp(rs.uniform(np.log(0.37), np.log(55.0), size=(H, W))).astype(F)
    if depth is not None:
        z = np.full((H, W), depth, F)
    nrm = rs.normal(size=(H, W, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=-1, keepdims=True)).astype(F)
    tri = rs.randint(0, 50, size=(H, W)).astype(np.int32)
    if blocks:
        ys, xs = np.mgrid[0:H, 0:W]
        three = np.asarray([[0.0, 1.0, 0.0], [0.6, 0.0, -0.8], [-0.8, 0.6, 0.0]], F)
        nrm = three[(xs // 16) % 3]
        tri = ((ys // 8) * 64 + xs // 8).astype(np.int32)
    miss = (rs.uniform(size=(H, W)) < miss_fraction) | ~in_frame(smp)
    z[miss] = INF
    nrm[miss] = 0
    tri[miss] = -1
    return dict(depth=z, normal=nrm, triangle=tri)


_cache = {}


def _frozen(key, make):
    if key not in _cache:
        out = make()
        for a in out[0] + tuple(out[1].values()) + tuple(out[3].values()):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _cache[key] = out
    return _cache[key]


def unmoved_case(kind, W, H, depth=None, rotated=False, fov=None):
    """-> (sums (fb, sq, count), aov_src, smp_src, aov_dst, smp_dst): one camera on both sides, counts <= 64"""
    def make():
        smp = sampler(kind, W, H, fov=fov, **(CAM_ROTATED if rotated else CAM_PLAIN))
        aov = guides(smp, 11 + W + H, depth)
        return rref.sums(W, H, 7, counts=(0, 1, 2, 7, 20, 64)), aov, smp, dict(aov), smp
    return _frozen(("unmoved", kind, W, H, depth, rotated, fov), make)


def moved_case(kind, W, H):
    """a small move with a yaw under guides of one depth, normals in bands and ids in blocks: taps of every kind
    (kept, rejected as a miss, by normal or by triangle, off the frame) occur — a case for GPU == host, not for
    a property"""
    def make():
        a = sampler(kind, W, H, **CAM_PLAIN)
        b = sampler(kind, W, H, pos=(0.28, -0.49, 1.03), yaw=0.013, pitch=-0.004, ortho_half_width=2.1,
                    fov=None if kind != "fisheye" else 2.9)
        aov_a = guides(a, 5, depth=4.0, blocks=True)
        aov_b = guides(b, 5, depth=4.0, blocks=True)  # (the same seed: the same pixels miss on both sides)
        return rref.sums(W, H, 9, counts=(0, 1, 2, 7, 20, 64, 300)), aov_a, a, aov_b, b
    return _frozen(("moved", kind, W, H), make)


def yaw_step(W):
    """the yaw of one equirect column, as the float32 the camera holds"""
    return F(TAU / F(W))


def column_shift(smp_src, smp_dst):
    """the k for which dst column x looks where src column x + k does, from the samplers' own centre rays"""
    W, H = smp_src.width, smp_src.height
    row = (H // 2) * W
    ds = rt.sampler_rays_host(smp_src)[row:row + W, 3:]
    dd = rt.sampler_rays_host(smp_dst)[row:row + W, 3:]
    k = int(np.argmax(ds.astype(np.float64) @ dd[0].astype(np.float64)))
    assert (ds[k].astype(np.float64) @ dd[0].astype(np.float64)) > 1.0 - 1e-6
    return k


def equirect_yaw_case(W, H, k):
    """an EQUIRECT camera yawed by k columns: the dst guides are the src guides rolled, so is the expected frame.
    -> (sums, aov_src, smp_src, aov_dst, smp_dst, shift) with dst[:, x] == src[:, (x + shift) % W]"""
    def make():
        a = sampler("equirect", W, H, pos=CAM_PLAIN["pos"])
        b = sampler("equirect", W, H, pos=CAM_PLAIN["pos"], yaw=float(F(k) * yaw_step(W)))
        shift = column_shift(a, b)
        aov_a = guides(a, 21 + k)
        aov_b = {n: np.roll(v, -shift, axis=1) for n, v in aov_a.items()}
        return rref.sums(W, H, 3, counts=(0, 1, 2, 7, 20, 64)), aov_a, a, aov_b, b, shift
    return _frozen(("yaw", W, H, k), make)


def ortho_shift_case(W, H, shift_px, dist=4.0, counts=None):
    """an ORTHO camera (yaw = pitch = 0, half width 2: a pixel is 4 / W units) moved `shift_px` pixels along its
    right axis over a fronto-parallel plane at `dist`"""
    ohw = 2.0
    a = sampler("ortho", W, H, pos=CAM_PLAIN["pos"], ortho_half_width=ohw)
    rays = rt.sampler_rays_host(a)
    px = rays[1, 0:3] - rays[0, 0:3]  # one pixel along the right axis, as the sampler lays the origins out
    pos = tuple(float(F(CAM_PLAIN["pos"][c]) + F(shift_px) * px[c]) for c in range(3))
    b = sampler("ortho", W, H, pos=pos, ortho_half_width=ohw)
    nrm = np.zeros((H, W, 3), F)
    nrm[..., 2] = -1
    aov = dict(depth=np.full((H, W), dist, F), normal=nrm, triangle=np.full((H, W), 5, np.int32))
    fb, sq, count = rref.sums(W, H, 5, counts=(1, 2, 7, 20, 64))
    if counts is not None:
        mean = fb / count[..., None].astype(F)
        count = np.broadcast_to(np.asarray(counts, np.int32), (H, W)).copy()
        fb = (mean * count[..., None].astype(F)).astype(F)
    return (fb, sq, count), aov, a, {n: v.copy() for n, v in aov.items()}, b


BAD_CAMERAS = {  # name -> (which side, camera fields): every pixel must reset
    "nan_position": ("dst", dict(pos=(float("nan"), -0.5, 1.0))),
    "inf_position": ("dst", dict(pos=(0.25, float("inf"), 1.0))),
    "inf_position_src": ("src", dict(pos=(float("-inf"), float("inf"), float("inf")))),
    "inf_yaw": ("dst", dict(pos=CAM_PLAIN["pos"], yaw=float("inf"))),
    "nan_pitch_src": ("src", dict(pos=CAM_PLAIN["pos"], pitch=float("nan"))),
    "huge_yaw": ("dst", dict(pos=CAM_PLAIN["pos"], yaw=float(2 ** 20))),
    "huge_pitch_src": ("src", dict(pos=CAM_PLAIN["pos"], pitch=float(2 ** 20))),
}


def bad_camera_case(kind, W, H, name):
    sums, aov_a, a, aov_b, b = unmoved_case(kind, W, H)
    side, fields = BAD_CAMERAS[name]
    bad = sampler(kind, W, H, **fields)
    return (sums, aov_a, bad, aov_b, b) if side == "src" else (sums, aov_a, a, aov_b, bad)


def roll_frame(f, k):
    """denoise_ref's frame dict rolled by k columns"""
    return {n: np.roll(v, k, axis=1) for n, v in f.items()}
