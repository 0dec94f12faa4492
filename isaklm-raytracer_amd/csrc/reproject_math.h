// reproject_math.h — the per-pixel arithmetic of rt_reproject, one text for
// the gfx950 kernel (reproject.hip) and the host tier (host/reproject_host.cpp).
//
// A backward reprojection of a frame's per-pixel sums (frame_buffer,
// squared_luminance, sample_count) to a moved camera, guided by the first-hit
// AOVs of both cameras (DESIGN.md "Temporal reprojection" has the whole
// definition).  As in denoise_math.h every operation is a correctly rounded
// float32 operation (+ - * / sqrtf floorf, compares) in the order written
// here, no fused operations (every includer is built with -ffp-contract=off),
// minima written as compares — so the GPU, the host and a restatement in any
// IEEE float32 arithmetic give the same bits.  The cameras' rotation and
// tan(FOV / 2) are host-side frame constants (camera_math.h).
//
// rt_reproject_sampler runs the same text for the samplers' other camera
// models (equirectangular, fisheye, orthographic): the model is a compile-time
// parameter, only the projection (steps 2 and 3) differs, and it adds
// rt_atan2f and rt_sincosf (rt_libm.h: the same bits on both sides) to the
// operations above.  The pinhole instantiation is rt_reproject's own.
#pragma once

#include <math.h>

#include "camera_math.h"
#include "sampler_math.h"

#define RT_RP_DEFAULT_MAX_HISTORY 64
#define RT_RP_DEFAULT_DEPTH_TOL 0.02f
#define RT_RP_DEFAULT_NORMAL_MIN 0.95f
#define RT_RP_MAX_HISTORY (1 << 20)
#define RT_RP_SNAP (1.0f / 64.0f)        // a projection this close to a pixel centre on both axes takes that pixel alone
#define RT_RP_MIN_WEIGHT (1.0f / 16.0f)  // the valid taps must hold at least this much of the bilinear weight

// the options with every default resolved
struct RtRpParams {
    int max_history;
    float depth_tol, normal_min;
    int match_triangle; // 1 / 0
};

// RtReprojectOptions (NULL = the defaults) -> RtRpParams; false: a value out of range
inline bool rt_rp_resolve(const RtReprojectOptions *opt, RtRpParams *p)
{
    RtReprojectOptions o = {0, 0.0f, 0.0f, 0, nullptr, nullptr};
    if (opt) o = *opt;
    p->max_history = o.max_history ? o.max_history : RT_RP_DEFAULT_MAX_HISTORY;
    p->depth_tol = o.depth_tol != 0.0f ? o.depth_tol : RT_RP_DEFAULT_DEPTH_TOL;
    p->normal_min = o.normal_min != 0.0f ? o.normal_min : RT_RP_DEFAULT_NORMAL_MIN;
    p->match_triangle = o.match_triangle >= 0;
    if (p->max_history < 1 || p->max_history > RT_RP_MAX_HISTORY) return false;
    if (o.match_triangle < -1 || o.match_triangle > 1) return false;
    // negative, NaN and infinite tolerances (a NaN fails both compares)
    if (!(p->depth_tol > 0.0f && p->depth_tol <= 3.0e38f)) return false;
    if (!(p->normal_min > -1.0f && p->normal_min <= 1.0f)) return false;
    return true;
}

// A camera's frame constants (host only): a NaN, infinite or absurd angle gives NaN constants (camera_math.h),
// which fail every compare of the projection, so every pixel resets.
inline RtDevCamera rt_rp_camera(const Camera &cam) { return rt_device_camera_checked(cam); }

// one frame's arrays: the sums (NULL on the new camera's side) and the guides
struct RtRpFrame {
    const Vec3D *fb;
    const float *sq;
    const int *count;
    const float *depth;
    const float *normal;
    const int *triangle; // may be NULL
};

struct RtRpPixel {
    Vec3D fb;
    float sq;
    int count;
};

RT_HD RtRpPixel rt_rp_reset()
{
    RtRpPixel o;
    o.fb = rt_v3(0.0f, 0.0f, 0.0f);
    o.sq = 0.0f;
    o.count = 0;
    return o;
}

RT_HD bool rt_rp_finite(float x) { return fabsf(x) < INFINITY; }

// The camera move's translation, computed once per call.
RT_HD Vec3D rt_rp_delta(const RtDevCamera &src_cam, const RtDevCamera &dst_cam)
{
    return rt_v3(dst_cam.pos[0] - src_cam.pos[0], dst_cam.pos[1] - src_cam.pos[1], dst_cam.pos[2] - src_cam.pos[2]);
}

// What the camera models beside the pinhole need of the two samplers (rt_reproject_sampler): the FISHEYE
// half angles and the ORTHO half widths.  rt_reproject's pinhole reads none of it.
struct RtRpLens {
    float src_half_fov, dst_half_fov;
    float src_ortho_half_width, dst_ortho_half_width;
};

inline RtRpLens rt_rp_lens(const RtDevSampler &src, const RtDevSampler &dst)
{
    RtRpLens l;
    l.src_half_fov = src.half_fov;
    l.dst_half_fov = dst.half_fov;
    l.src_ortho_half_width = src.ortho_half_width;
    l.dst_ortho_half_width = dst.ortho_half_width;
    return l;
}

// Steps 2 and 3 for the models beside the pinhole: the point seen through dst pixel (x, y) at depth z, relative to
// the old camera, and where that camera's model sees it — the continuous source pixel (u, w) and the depth z_exp
// the source's AOV holds there.  false: the old camera does not see the point (or a NaN / an infinity came by).
//
// The centre ray is the sampler's own text (sampler_math.h rt_sampler_ray<true>) run for a camera at the origin,
// so d has the bits of rt_sample_aov's ray and the origin comes out relative to the camera position:
// o_rel = +0 for EQUIRECT and FISHEYE, (0 + R*(u, 0, 0)) + R*(0, v, 0) for ORTHO.  Then, in this order,
//   v = (delta + o_rel) + d * z;   c = (v . Rs.i, v . Rs.j, v . Rs.k);   |v| = sqrtf((v.x^2 + v.y^2) + v.z^2)
//   ORTHO     z_exp = c.z, which must be > 0;  u = (c.x / ohw * (W * 0.5) + W * 0.5) - 0.5;
//             w = (c.y / ohw * (W * 0.5) + H * 0.5) - 0.5            (ohw: the source's ortho_half_width)
//   EQUIRECT  z_exp = |v|;  lon = atan2(c.x, c.z);  h = sqrtf(c.x^2 + c.z^2);  lat = atan2(c.y, h);
//             u = (lon + PI) / TAU * W - 0.5;  w = (lat + PI * 0.5) / PI * H - 0.5
//   FISHEYE   z_exp = |v|;  h = sqrtf(c.x^2 + c.y^2);  theta = atan2(h, c.z);  r = theta / half_fov, which must be
//             <= 1;  s = h > 0 ? r / h : 0;  rad = min(W, H) * 0.5;  u = ((s * c.x) * rad + W * 0.5) - 0.5;
//             w = ((s * c.y) * rad + H * 0.5) - 0.5                  (half_fov: the source's FOV * 0.5)
// with atan2 = rt_atan2f (rt_libm.h), PI and TAU sampler_math.h's, W, H = (float)width, height.  z_exp must be
// > 0 and finite for every model: an infinite camera position gives an infinite |v|, whose angles are finite and
// whose depth test every tap would pass.
template <int MODEL>
RT_HD bool rt_rp_project(const RtDevCamera &src_cam, const RtDevCamera &dst_cam, const RtRpLens &lens, Vec3D delta,
                         int width, int height, int x, int y, float z, float &u, float &w, float &z_exp)
{
    static_assert(MODEL == RT_SAMPLER_EQUIRECT || MODEL == RT_SAMPLER_FISHEYE || MODEL == RT_SAMPLER_ORTHO,
                  "the pinhole's projection is rt_rp_pixel's own");
    RtDevSampler s;
    s.kind = MODEL;
    s.width = width;
    s.height = height;
    s.half_w = s.half_h = 0;
    s.cam = dst_cam;
    s.cam.pos[0] = s.cam.pos[1] = s.cam.pos[2] = 0.0f;
    s.half_fov = lens.dst_half_fov;
    s.ortho_half_width = lens.dst_ortho_half_width;
    s.pixels = nullptr;
    s.points = nullptr;
    uint32_t st = 0;
    Vec3D o_rel, d;
    rt_sampler_ray<true>(s, (uint32_t)y * (uint32_t)width + (uint32_t)x, st, o_rel, d);
    const Vec3D v = rt_v3((delta.x + o_rel.x) + d.x * z, (delta.y + o_rel.y) + d.y * z, (delta.z + o_rel.z) + d.z * z);
    const RtM3 Rs = rt_camera_rotation(src_cam);
    const float cx = rt_dot(v, Rs.i), cy = rt_dot(v, Rs.j), cz = rt_dot(v, Rs.k);
    const float W = (float)width, H = (float)height;
    if (MODEL == RT_SAMPLER_ORTHO) {
        z_exp = cz;
        u = (cx / lens.src_ortho_half_width * (W * 0.5f) + W * 0.5f) - 0.5f;
        w = (cy / lens.src_ortho_half_width * (W * 0.5f) + H * 0.5f) - 0.5f;
    } else {
        z_exp = sqrtf((v.x * v.x + v.y * v.y) + v.z * v.z);
        if (MODEL == RT_SAMPLER_EQUIRECT) {
            const float lon = rt_atan2f(cx, cz);
            const float h = sqrtf(cx * cx + cz * cz);
            const float lat = rt_atan2f(cy, h);
            u = (lon + RT_PI) / RT_TAU * W - 0.5f;
            w = (lat + RT_PI * 0.5f) / RT_PI * H - 0.5f;
        } else {
            const float h = sqrtf(cx * cx + cy * cy);
            const float theta = rt_atan2f(h, cz);
            const float r = theta / lens.src_half_fov;
            if (!(r <= 1.0f)) return false; // outside the image circle (or a NaN)
            const float sc = h > 0.0f ? r / h : 0.0f;
            const float rad = (width < height ? W : H) * 0.5f;
            u = ((sc * cx) * rad + W * 0.5f) - 0.5f;
            w = ((sc * cy) * rad + H * 0.5f) - 0.5f;
        }
    }
    return z_exp > 0.0f && z_exp < INFINITY; // (a NaN fails)
}

// Output pixel (x, y) of the new camera's frame.  MODEL: the two cameras' model, RT_SAMPLER_PINHOLE ..
// RT_SAMPLER_ORTHO; the pinhole (rt_reproject, and rt_reproject_sampler's PINHOLE) reads no lens.
template <int MODEL = RT_SAMPLER_PINHOLE>
RT_HD RtRpPixel rt_rp_pixel(const RtRpFrame &src, const RtDevCamera &src_cam, const float *dst_depth,
                            const float *dst_normal, const int *dst_triangle, const RtDevCamera &dst_cam,
                            Vec3D delta, int width, int height, int x, int y, const RtRpParams &prm,
                            const RtRpLens &lens = RtRpLens{0.0f, 0.0f, 0.0f, 0.0f})
{
    const size_t p = (size_t)y * width + x;
    // 1. a miss is black: nothing to carry
    const float z = dst_depth[p];
    if (!(z < INFINITY)) return rt_rp_reset();
    float u, w, z_exp;
    if constexpr (MODEL == RT_SAMPLER_PINHOLE) {
        // 2. the first hit relative to the old camera (never a world position: |position| would cancel)
        const int half_w = width / 2, half_h = height / 2;
        const Vec3D d = rt_camera_centre_dir(dst_cam, half_w, half_h, x, y);
        const Vec3D v = rt_v3(delta.x + d.x * z, delta.y + d.y * z, delta.z + d.z * z);
        // 3. its projection into the old camera
        const RtM3 Rs = rt_camera_rotation(src_cam);
        const float cx = rt_dot(v, Rs.i), cy = rt_dot(v, Rs.j), cz = rt_dot(v, Rs.k);
        if (!(cz > 0.0f)) return rt_rp_reset();
        u = (cx / cz) / src_cam.tan_half_fov * (float)half_w + (float)half_w - 0.5f;
        w = (cy / cz) / src_cam.tan_half_fov * (float)half_w + (float)half_h - 0.5f;
        if (!(u > -1.0f && u < (float)width && w > -1.0f && w < (float)height)) return rt_rp_reset(); // (a NaN fails)
        z_exp = sqrtf((v.x * v.x + v.y * v.y) + v.z * v.z);
    } else {
        // 2., 3. the same for the other models (rt_rp_project)
        if (!rt_rp_project<MODEL>(src_cam, dst_cam, lens, delta, width, height, x, y, z, u, w, z_exp)) return rt_rp_reset();
        if (!(u > -1.0f && u < (float)width && w > -1.0f && w < (float)height)) return rt_rp_reset(); // (a NaN fails)
    }
    const float z_tol = prm.depth_tol * z_exp;
    // 4. the taps: one at a pixel centre, else the four bilinear ones
    const float ru = floorf(u + 0.5f), rw = floorf(w + 0.5f);
    const bool snap = fabsf(u - ru) <= RT_RP_SNAP && fabsf(w - rw) <= RT_RP_SNAP;
    int tx[4], ty[4];
    float tw[4];
    int taps;
    if (snap) {
        taps = 1;
        tx[0] = (int)ru;
        ty[0] = (int)rw;
        tw[0] = 1.0f;
        for (int t = 1; t < 4; ++t) {
            tx[t] = ty[t] = 0;
            tw[t] = 0.0f;
        }
    } else {
        taps = 4;
        const float fu = floorf(u), fw = floorf(w);
        const int x0 = (int)fu, y0 = (int)fw;
        const float ax = u - fu, ay = w - fw;
        const float bx = 1.0f - ax, by = 1.0f - ay;
        tx[0] = x0;     ty[0] = y0;     tw[0] = bx * by;
        tx[1] = x0 + 1; ty[1] = y0;     tw[1] = ax * by;
        tx[2] = x0;     ty[2] = y0 + 1; tw[2] = bx * ay;
        tx[3] = x0 + 1; ty[3] = y0 + 1; tw[3] = ax * ay;
    }
    if constexpr (MODEL == RT_SAMPLER_EQUIRECT) {
        // longitude is periodic: columns -1 and width (u lies in (-1, width)) are columns width - 1 and 0; rows
        // are not wrapped (the poles are edges)
        for (int t = 0; t < 4; ++t) tx[t] = tx[t] < 0 ? tx[t] + width : (tx[t] >= width ? tx[t] - width : tx[t]);
    }
    // 5. validity, cheapest guide first: the colour of a rejected tap is never loaded
    const float *np = dst_normal + 3 * p;
    const Vec3D n_p = rt_v3(np[0], np[1], np[2]);
    const bool match = prm.match_triangle && src.triangle && dst_triangle;
    const int tri_p = match ? dst_triangle[p] : 0;
    size_t tq[4];
    int tn[4];
    bool ok[4];
    float wsum = 0.0f;
    int n_h = 0x7fffffff;
    for (int t = 0; t < 4; ++t) { // (a constant trip count: the tap arrays stay in registers)
        ok[t] = false;
        tn[t] = 0;
        tq[t] = 0;
        if (t >= taps) continue;
        if (tx[t] < 0 || tx[t] >= width || ty[t] < 0 || ty[t] >= height) continue;
        const size_t q = (size_t)ty[t] * width + tx[t];
        const int n = src.count[q];
        if (n <= 0) continue;
        const float zq = src.depth[q];
        if (!(zq < INFINITY)) continue;
        if (!(fabsf(zq - z_exp) <= z_tol)) continue;
        const float *nq = src.normal + 3 * q;
        if (!(rt_dot(n_p, rt_v3(nq[0], nq[1], nq[2])) >= prm.normal_min)) continue;
        if (match && src.triangle[q] != tri_p) continue;
        ok[t] = true;
        tq[t] = q;
        tn[t] = n;
        wsum += tw[t];
        if (n < n_h) n_h = n;
    }
    // 6. enough of the footprint must be the same surface
    if (!(wsum >= RT_RP_MIN_WEIGHT)) return rt_rp_reset();
    if (prm.max_history < n_h) n_h = prm.max_history;
    // 7. the carried sums
    RtRpPixel o;
    o.count = n_h;
    if (snap && n_h == tn[0]) { // the same pixel, its whole history: the sums themselves
        o.fb = src.fb[tq[0]];
        o.sq = src.sq[tq[0]];
    } else {
        float mx = 0.0f, my = 0.0f, mz = 0.0f, ms = 0.0f;
        for (int t = 0; t < 4; ++t) {
            if (!ok[t]) continue;
            const Vec3D f = src.fb[tq[t]];
            const float fn = (float)tn[t];
            const float inv = 1.0f / fn;
            mx += tw[t] * (f.x * inv);
            my += tw[t] * (f.y * inv);
            mz += tw[t] * (f.z * inv);
            ms += tw[t] * (src.sq[tq[t]] / fn);
        }
        const float nf = (float)n_h;
        o.fb = rt_v3(mx / wsum * nf, my / wsum * nf, mz / wsum * nf);
        o.sq = ms / wsum * nf;
    }
    // a NaN or Inf sum would spread through the taps of every later frame: such a pixel starts again
    if (!(rt_rp_finite(o.fb.x) && rt_rp_finite(o.fb.y) && rt_rp_finite(o.fb.z) && rt_rp_finite(o.sq))) return rt_rp_reset();
    return o;
}
