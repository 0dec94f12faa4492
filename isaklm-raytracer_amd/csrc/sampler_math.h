// sampler_math.h — the RNG step and the ray samplers of rt_sample_paths /
// rt_sampler_rays, one text for the gfx950 kernels (query.hip) and the host
// twin (host/sampler_host.cpp).
//
// A sampler maps (element e, RNG state st) to (origin o, direction d, new st):
// DESIGN.md §11 "Samplers" has the definition operation by operation.  As in
// camera_math.h, denoise_math.h and reproject_math.h every operation is a
// correctly rounded float32 operation (+ - * / sqrtf copysignf, compares) or
// rt_sincosf (rt_libm.h) in the order written here, no fused operations (every
// includer is built with -ffp-contract=off) — so the GPU, the host and a
// restatement in any IEEE float32 arithmetic give the same bits.  No float is
// converted to an int and nothing is indexed by a float; rt_sincosf only ever
// sees a finite angle of a few radians (a jitter draw times a constant, or
// r <= 1 times a validated FOV), whatever the camera holds.
#pragma once

#include <math.h>
#include <stdint.h>

#include "camera_math.h"

// get_random_unilateral (rt/path_tracing.cuh:34-43): the one definition of the RNG step (rt_kernels.h rng_next
// forwards here)
RT_HD float rt_rng_next(uint32_t &st)
{
    uint32_t state = st * 747796405u + 2891336453u;
    uint32_t word = ((state >> ((state >> 28u) + 4u)) ^ state) * 277803737u;
    uint32_t r = (word >> 22u) ^ word;
    st = r;
    return (float)r / (float)UINT32_MAX;
}

// RtSampler with its frame constants resolved on the host (rt_sampler_resolve)
struct RtDevSampler {
    int kind;               // RT_SAMPLER_*
    int width, height;      // image kinds
    int half_w, half_h;     // PINHOLE: width / 2, height / 2 (integer division), as rt_render's frame
    RtDevCamera cam;        // image kinds
    float half_fov;         // FISHEYE: FOV * 0.5f
    float ortho_half_width; // ORTHO
    const int32_t *pixels;  // image kinds, optional
    const float *points;    // HEMISPHERE: n x 6 floats
};

// RtSampler -> RtDevSampler for n elements; nullptr, or the text of the rule that failed (host only)
inline const char *rt_sampler_resolve(const RtSampler *s, long long n, RtDevSampler *out)
{
    if (!s) return "null sampler";
    if (s->kind < RT_SAMPLER_PINHOLE || s->kind > RT_SAMPLER_HEMISPHERE) return "kind out of range";
    RtDevSampler d;
    d.kind = s->kind;
    d.width = d.height = d.half_w = d.half_h = 0;
    d.half_fov = 0.0f;
    d.ortho_half_width = 0.0f;
    d.pixels = nullptr;
    d.points = nullptr;
    Camera cam = s->camera;
    if (s->kind != RT_SAMPLER_PINHOLE) cam.FOV = 0.0f; // (its tangent is the pinhole's alone)
    if (s->kind == RT_SAMPLER_HEMISPHERE) {
        if (!s->points_device || ((uintptr_t)s->points_device & 7)) return "null or misaligned points (8 B)";
        d.points = s->points_device;
        cam.yaw = cam.pitch = 0.0f; // (no camera)
        d.cam = rt_device_camera_checked(cam);
        *out = d;
        return nullptr;
    }
    if (s->width < 1 || s->height < 1 || (long long)s->width * s->height > (1LL << 31) - 1) return "bad frame size";
    if ((uintptr_t)s->pixels_device & 3) return "misaligned pixel list (4 B)";
    if (!s->pixels_device && n != (long long)s->width * s->height) return "no pixel list and n != width * height";
    if (s->kind == RT_SAMPLER_FISHEYE && !(s->camera.FOV > 0.0f && s->camera.FOV <= RT_TAU))
        return "fisheye FOV outside (0, 2 pi]"; // (a NaN fails the first compare)
    if (s->kind == RT_SAMPLER_ORTHO && !(s->ortho_half_width > 0.0f && s->ortho_half_width <= 3.4028234e38f))
        return "ortho_half_width not finite or <= 0";
    d.width = s->width;
    d.height = s->height;
    d.half_w = s->width / 2;
    d.half_h = s->height / 2;
    d.cam = rt_device_camera_checked(cam);
    d.half_fov = s->camera.FOV * 0.5f;
    d.ortho_half_width = s->ortho_half_width;
    d.pixels = s->pixels_device;
    *out = d;
    return nullptr;
}

// A sampler that stands for a whole frame (rt_denoise_sampler, rt_reproject_sampler): an image kind without a
// pixel list; nullptr, or the text of the rule that failed (host only)
inline const char *rt_sampler_resolve_frame(const RtSampler *s, RtDevSampler *out)
{
    if (!s) return "null sampler";
    if (s->kind == RT_SAMPLER_HEMISPHERE) return "a hemisphere sampler has no frame";
    if (s->pixels_device) return "a pixel list is not a whole frame";
    return rt_sampler_resolve(s, (long long)s->width * s->height, out);
}

// the branch-free orthonormal frame of n (Duff et al. 2017, "Building an Orthonormal Basis, Revisited")
RT_HD void rt_sampler_frame(Vec3D n, Vec3D &t, Vec3D &b)
{
    const float sg = copysignf(1.0f, n.z);
    const float a = -1.0f / (sg + n.z);
    const float q = n.x * n.y * a;
    t = rt_v3(1.0f + sg * n.x * n.x * a, sg * q, -sg * n.x);
    b = rt_v3(q, sg + n.y * n.y * a, -n.y);
}

// Element e's next ray.  CENTRE (image kinds): both jitter draws are 0.5, no lens offset, nothing drawn.
template <bool CENTRE>
RT_HD void rt_sampler_ray(const RtDevSampler &s, uint32_t e, uint32_t &st, Vec3D &o, Vec3D &d)
{
    if (s.kind == RT_SAMPLER_HEMISPHERE) {
        const float *p = s.points + 6 * (size_t)e;
        const Vec3D n = rt_v3(p[3], p[4], p[5]);
        o = rt_v3(p[0], p[1], p[2]);
        // diffuse_direction's draws and arithmetic (rt_kernels.h scatter; rt/path_tracing.cuh:45-59)
        const float dphi = rt_rng_next(st) * RT_TAU;
        float ds, dc;
        rt_sincosf(dphi, &ds, &dc);
        const float ru2 = rt_rng_next(st);
        const float sq = sqrtf(ru2);
        Vec3D t, b;
        rt_sampler_frame(n, t, b);
        d = sq * dc * t + sqrtf(1.0f - ru2) * n + sq * ds * b;
        return;
    }
    uint32_t pi = e;
    if (s.pixels) pi = (uint32_t)s.pixels[e];
    if (pi >= (uint32_t)s.width * (uint32_t)s.height) { // outside the frame: a ray that hits nothing, no draw
        o = d = rt_v3(0.0f, 0.0f, 0.0f);
        return;
    }
    const float fx = (float)(pi % (uint32_t)s.width), fy = (float)(pi / (uint32_t)s.width);
    const float W = (float)s.width, H = (float)s.height;
    const RtM3 R = rt_camera_rotation(s.cam);
    const Vec3D pos = rt_v3(s.cam.pos[0], s.cam.pos[1], s.cam.pos[2]);
    const float rx = CENTRE ? 0.5f : rt_rng_next(st);
    const float ry = CENTRE ? 0.5f : rt_rng_next(st);
    if (s.kind == RT_SAMPLER_PINHOLE) { // camera_ray (rt_kernels.h; rt/path_tracing.cuh:381-391, :327-336)
        const float hw = (float)s.half_w, hh = (float)s.half_h;
        const Vec3D dir = rt_normalize(
            rt_v3(s.cam.tan_half_fov * (fx + rx - hw) / hw, s.cam.tan_half_fov * (fy + ry - hh) / hw, 1.0f));
        d = R * dir;
        o = pos;
        if (!CENTRE) {
            const float theta = rt_rng_next(st) * RT_TAU;
            const float r = sqrtf(rt_rng_next(st)) * s.cam.aperture;
            float sn, cs;
            rt_sincosf(theta, &sn, &cs);
            const float ox = r * cs;
            const float oy = r * sn;
            o = pos + R * rt_v3(ox, 0.0f, 0.0f) + R * rt_v3(0.0f, oy, 0.0f);
        }
    } else if (s.kind == RT_SAMPLER_EQUIRECT) {
        const float lon = (fx + rx) / W * RT_TAU - RT_PI;
        const float lat = (fy + ry) / H * RT_PI - RT_PI * 0.5f;
        float sl, cl, sa, ca;
        rt_sincosf(lon, &sl, &cl);
        rt_sincosf(lat, &sa, &ca);
        d = R * rt_v3(ca * sl, sa, ca * cl);
        o = pos;
    } else if (s.kind == RT_SAMPLER_FISHEYE) { // equidistant, the image circle inscribed in the shorter side
        const float rad = (s.width < s.height ? W : H) * 0.5f;
        const float u = ((fx + rx) - W * 0.5f) / rad;
        const float v = ((fy + ry) - H * 0.5f) / rad;
        const float r = sqrtf(u * u + v * v);
        o = pos;
        if (!(r <= 1.0f)) { // outside the circle (or a NaN)
            d = rt_v3(0.0f, 0.0f, 0.0f);
        } else {
            const float theta = r * s.half_fov;
            float sn, cs;
            rt_sincosf(theta, &sn, &cs);
            const float k = r > 0.0f ? sn / r : 0.0f;
            d = R * rt_v3(k * u, k * v, cs);
        }
    } else { // RT_SAMPLER_ORTHO: square pixels, the half width across W / 2 of them
        const float u = ((fx + rx) - W * 0.5f) / (W * 0.5f) * s.ortho_half_width;
        const float v = ((fy + ry) - H * 0.5f) / (W * 0.5f) * s.ortho_half_width;
        o = (pos + R * rt_v3(u, 0.0f, 0.0f)) + R * rt_v3(0.0f, v, 0.0f);
        d = R * rt_v3(0.0f, 0.0f, 1.0f);
    }
}
