"""A numpy restatement of rt_denoise's filter, written from its definition
(DESIGN.md "Denoising"), not from csrc/denoise_math.h: float32 arrays
throughout, one numpy operation per stated operation, the 25 taps
accumulated one after the other in the stated order (vectorised across
pixels, never across taps).  IEEE float32 + - * / sqrt are correctly rounded
in numpy as on the GPU, so the library must give the same bits.

Also the seeded synthetic frames the denoiser's tests share."""
import numpy as np

F = np.float32
INF = F(np.inf)
K5 = (F(3 / 8), F(1 / 4), F(1 / 16))  # the 5-tap B3 spline, by |offset|
G3 = (F(1 / 2), F(1 / 4))             # the 3-tap binomial, by |offset|

DEFAULTS = dict(iterations=5, sigma_lum=4.0, sigma_depth=1.0, normal_log2=7, demodulate=True)


def _lum(r, g, b):
    return (r * F(0.2126) + g * F(0.7152)) + b * F(0.0722)


def _max0(x):
    return np.where(x > 0, x, F(0))


def _falloff(x):
    r = F(1) / (F(1) + x * x)
    return r * r


def _shift(a, dy, dx):
    """a[y + dy, x + dx] with indices clamped to the frame, and the mask of taps inside it"""
    H, W = a.shape[:2]
    ys, xs = np.arange(H) + dy, np.arange(W) + dx
    valid = ((ys >= 0) & (ys < H))[:, None] & ((xs >= 0) & (xs < W))[None, :]
    return a[np.clip(ys, 0, H - 1)][:, np.clip(xs, 0, W - 1)], valid


def _axis_slope(z, hit, dy, dx):
    zn, vn = _shift(z, dy, dx)
    zp, vp = _shift(z, -dy, -dx)
    hn, _ = _shift(hit, dy, dx)
    hp, _ = _shift(hit, -dy, -dx)
    use_n, use_p = vn & hn, vp & hp
    a, b = np.abs(zn - z), np.abs(z - zp)
    return np.where(use_n & use_p, np.where(b < a, b, a), np.where(use_n, a, np.where(use_p, b, F(0))))


def denoise(fb, sq, count, depth, normal, albedo, iterations=0, sigma_lum=0.0, sigma_depth=0.0, normal_log2=0,
            demodulate=True):
    """fb (H, W, 3), sq (H, W), count (H, W) int, depth (H, W), normal / albedo (H, W, 3) -> (H, W, 3) float32"""
    iterations = iterations or DEFAULTS["iterations"]
    sigma_lum = F(sigma_lum or DEFAULTS["sigma_lum"])
    sigma_depth = F(sigma_depth or DEFAULTS["sigma_depth"])
    normal_log2 = normal_log2 or DEFAULTS["normal_log2"]
    fb, sq, depth, normal = (np.asarray(a, F) for a in (fb, sq, depth, normal))
    H, W = depth.shape
    fb, normal, sq = fb.reshape(H, W, 3), normal.reshape(H, W, 3), sq.reshape(H, W)
    n = np.asarray(count, np.int32).reshape(H, W)
    with np.errstate(all="ignore"):
        # ---- prepare
        nf = n.astype(F)
        inv = F(1) / nf
        c = np.where((n > 0)[..., None], fb * inv[..., None], F(0))
        if demodulate:
            albedo = np.asarray(albedo, F).reshape(H, W, 3)
            den = np.where(albedo >= F(1 / 1024), albedo, F(1))
        else:
            den = np.ones((H, W, 3), F)
        irr = c / den
        tl = _lum(fb[..., 0], fb[..., 1], fb[..., 2])
        var_n = _max0((sq - (tl * tl) / nf) / (n - 1).astype(F)) / nf
        lc = _lum(c[..., 0], c[..., 1], c[..., 2])
        var = np.where(n >= 2, var_n, lc * lc)
        ld = _lum(den[..., 0], den[..., 1], den[..., 2])
        v = var / (ld * ld)
        hit = depth < INF
        gx = _axis_slope(depth, hit, 0, 1)
        gy = _axis_slope(depth, hit, 1, 0)
        gz = np.where(gx > gy, gx, gy)
        # ---- the a-trous levels
        for s in range(iterations):
            step = 1 << s
            vbar = np.zeros((H, W), F)
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    vq, _ = _shift(v, dy, dx)
                    vbar = vbar + (G3[abs(dx)] * G3[abs(dy)]) * vq
            sd = sigma_lum * np.sqrt(_max0(vbar)) + F(1e-6)
            lum_p = _lum(irr[..., 0], irr[..., 1], irr[..., 2])
            sum_c = np.zeros((H, W, 3), F)
            sum_v = np.zeros((H, W), F)
            sum_w = np.zeros((H, W), F)
            for dy in (-2, -1, 0, 1, 2):
                for dx in (-2, -1, 0, 1, 2):
                    irr_q, valid = _shift(irr, step * dy, step * dx)
                    if not valid.any():
                        continue
                    v_q, _ = _shift(v, step * dy, step * dx)
                    n_q, _ = _shift(normal, step * dy, step * dx)
                    z_q, _ = _shift(depth, step * dy, step * dx)
                    hit_q, _ = _shift(hit, step * dy, step * dx)
                    h = K5[abs(dx)] * K5[abs(dy)]
                    d = (normal[..., 0] * n_q[..., 0] + normal[..., 1] * n_q[..., 1]) + normal[..., 2] * n_q[..., 2]
                    wn = _max0(d)
                    for _ in range(normal_log2):
                        wn = wn * wn
                    wz = _falloff(np.abs(depth - z_q) /
                                  (((sigma_depth * gz) * F((abs(dx) + abs(dy)) * step) + F(1e-4) * depth) + F(1e-30)))
                    wl = _falloff(np.abs(lum_p - _lum(irr_q[..., 0], irr_q[..., 1], irr_q[..., 2])) / sd)
                    w = np.where(hit != hit_q, F(0), np.where(~hit, h * wl, ((h * wn) * wz) * wl)).astype(F)
                    sum_c = np.where(valid[..., None], sum_c + w[..., None] * irr_q, sum_c)
                    sum_v = np.where(valid, sum_v + (w * w) * v_q, sum_v)
                    sum_w = np.where(valid, sum_w + w, sum_w)
            ok = sum_w > 0  # (a hit with a degenerate normal has no weight at all: it keeps its state)
            irr = np.where(ok[..., None], sum_c / sum_w[..., None], irr)
            v = np.where(ok, sum_v / (sum_w * sum_w), v)
        out = irr * den
    assert out.dtype == F
    return out


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def synthetic_frame(W, H, seed=1):
    """A seeded frame with every case of the filter: counts in {0, 1, 2, 7, 64} with a whole row of 0 (a row
    another shard owns), two tilted planes meeting at a vertical crease, a band of misses (+inf depth, normal
    and albedo 0), albedo channels below and above 1/1024.  Returns a dict of (H, W[, 3]) arrays."""
    rng = np.random.default_rng(seed * 7919 + W * 131 + H)
    count = rng.choice(np.array([0, 1, 2, 7, 64], np.int32), size=(H, W)).astype(np.int32)
    count[H // 2, :] = 0
    mean = rng.uniform(0.0, 2.0, size=(H, W, 3)).astype(F)
    fb = (mean * count[..., None].astype(F)).astype(F)
    fb[count == 0] = 0
    # sq ~ sum of squared sample luminances: n * (mean_lum^2 + spread), so the variance is positive and uneven
    ml = _lum(mean[..., 0], mean[..., 1], mean[..., 2])
    sq = (count.astype(F) * (ml * ml + rng.uniform(0.0, 1.0, size=(H, W)).astype(F))).astype(F)
    ys, xs = np.mgrid[0:H, 0:W]
    left = xs < (W + 1) // 2
    depth = np.where(left, 3.0 + 0.05 * xs + 0.02 * ys, 5.0 - 0.04 * xs + 0.03 * ys).astype(F)
    nl = np.array([-0.6, 0.0, 0.8], F)
    nr = np.array([0.8, 0.0, 0.6], F)
    normal = np.where(left[..., None], nl, nr).astype(F)
    albedo = rng.uniform(0.05, 0.95, size=(H, W, 3)).astype(F)
    albedo[rng.random((H, W, 3)) < 0.15] = F(1 / 2048)  # below the demodulation floor
    albedo[rng.random((H, W, 3)) < 0.05] = F(0)
    miss = (ys >= (2 * H) // 3) & (ys < (2 * H) // 3 + max(1, H // 6)) if H >= 3 else np.zeros((H, W), bool)
    depth[miss] = INF
    normal[miss] = 0
    albedo[miss] = 0
    return dict(fb=fb, sq=sq, count=count, depth=depth, normal=normal, albedo=albedo)


_cache = {}


def case(W, H, name):
    """(the synthetic frame of this shape, the restatement's output for the option set `name`): computed once,
    shared by the CPU and GPU tests, never modified (the arrays are read-only)"""
    key = (W, H, name)
    if key not in _cache:
        fkey = (W, H, None)
        if fkey not in _cache:
            f = synthetic_frame(W, H)
            for a in f.values():
                a.setflags(write=False)
            _cache[fkey] = f
        f = _cache[fkey]
        out = denoise(f["fb"], f["sq"], f["count"], f["depth"], f["normal"], f["albedo"], **OPTION_SETS[name])
        out.setflags(write=False)
        _cache[key] = (f, out)
    return _cache[key]


SHAPES = [(1, 1), (3, 2), (37, 29), (64, 48)]  # (W, H)
OPTION_SETS = {
    "defaults": {},
    "iterations1": dict(iterations=1),
    "iterations8": dict(iterations=8),
    "no_demodulation": dict(demodulate=False),
    "normal_log2_1": dict(normal_log2=1),
}
