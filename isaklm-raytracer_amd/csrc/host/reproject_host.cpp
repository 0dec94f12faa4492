// reproject_host.cpp — rt_reproject_host and rt_reproject_sampler_host:
// rt_reproject's arithmetic (reproject_math.h, the text the kernel compiles,
// one instantiation per camera model) on host arrays.  The CPU
// tier of the reprojection's tests, and the fall-back of an integrator without
// a GPU at hand: bit-identical to the GPU.  Depends on nothing but
// reproject_math.h.
#include "../reproject_math.h"

void rt_set_error(const char *fmt, ...);

extern "C" void rt_default_reproject_options(RtReprojectOptions *o)
{
    if (!o) return;
    o->max_history = RT_RP_DEFAULT_MAX_HISTORY;
    o->depth_tol = RT_RP_DEFAULT_DEPTH_TOL;
    o->normal_min = RT_RP_DEFAULT_NORMAL_MIN;
    o->match_triangle = 1;
    o->stream = nullptr;
    o->stats_device = nullptr;
}

// [a, a + na) and [b, b + nb) share a byte
bool rt_rp_ranges_overlap(const void *a, size_t na, const void *b, size_t nb)
{
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + nb && b0 < a0 + na;
}

// true: one of dst's three arrays shares a byte with one of src's three (n pixels each)
bool rt_rp_frames_overlap(const void *src_fb, const void *src_sq, const void *src_count, const void *dst_fb,
                          const void *dst_sq, const void *dst_count, size_t n)
{
    const void *s[3] = {src_fb, src_sq, src_count};
    const void *d[3] = {dst_fb, dst_sq, dst_count};
    const size_t bytes[3] = {n * sizeof(Vec3D), n * sizeof(float), n * sizeof(int)};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            if (rt_rp_ranges_overlap(s[i], bytes[i], d[j], bytes[j])) return true;
    return false;
}

// The two samplers of rt_reproject_sampler: whole frames of one image kind and size (the cameras, the FOV and
// ortho_half_width may differ); nullptr, or the text of the rule that failed
const char *rt_rp_resolve_samplers(const RtSampler *src, const RtSampler *dst, RtDevSampler *s, RtDevSampler *d)
{
    if (const char *why = rt_sampler_resolve_frame(src, s)) return why;
    if (const char *why = rt_sampler_resolve_frame(dst, d)) return why;
    if (s->kind != d->kind || s->width != d->width || s->height != d->height)
        return "the two samplers differ in kind, width or height";
    return nullptr;
}

namespace {

// every pixel of the new frame, on checked arguments
template <int MODEL>
void reproject_frame(const RtRpFrame &src, const RtDevCamera &sc, const float *dst_depth, const float *dst_normal,
                     const int32_t *dst_triangle, const RtDevCamera &dc, const RtRpLens &lens, int width, int height,
                     const RtRpParams &prm, float *dst_fb, float *dst_sq, int *dst_count, unsigned long long stats[3])
{
    const Vec3D delta = rt_rp_delta(sc, dc);
    unsigned long long kept = 0, samples = 0;
#pragma omp parallel for schedule(static) reduction(+ : kept, samples)
    for (int y = 0; y < height; ++y)
        for (int x = 0; x < width; ++x) {
            const size_t p = (size_t)y * width + x;
            const RtRpPixel o = rt_rp_pixel<MODEL>(src, sc, dst_depth, dst_normal, dst_triangle, dc, delta, width,
                                                   height, x, y, prm, lens);
            dst_fb[3 * p] = o.fb.x;
            dst_fb[3 * p + 1] = o.fb.y;
            dst_fb[3 * p + 2] = o.fb.z;
            dst_sq[p] = o.sq;
            dst_count[p] = o.count;
            kept += o.count > 0;
            samples += (unsigned long long)o.count;
        }
    if (stats) {
        stats[0] = (unsigned long long)width * height;
        stats[1] = kept;
        stats[2] = samples;
    }
}

// the options, the buffers and the overlap rule both host calls check (the frame size is checked before);
// who: the entry point's name
int check_arguments(const char *who, const float *src_fb, const float *src_sq, const int *src_count,
                    const float *src_depth, const float *src_normal, const float *dst_depth, const float *dst_normal,
                    int width, int height, float *dst_fb, float *dst_sq, int *dst_count)
{
    if (!src_fb || !src_sq || !src_count || !src_depth || !src_normal || !dst_depth || !dst_normal || !dst_fb ||
        !dst_sq || !dst_count) {
        rt_set_error("%s: null buffer", who);
        return RT_E_INVALID;
    }
    if (width < 1 || height < 1 || (long long)width * height > (1LL << 31) - 1) {
        rt_set_error("%s: bad frame size %d x %d", who, width, height);
        return RT_E_INVALID;
    }
    if (rt_rp_frames_overlap(src_fb, src_sq, src_count, dst_fb, dst_sq, dst_count, (size_t)width * height)) {
        rt_set_error("%s: dst overlaps src", who);
        return RT_E_INVALID;
    }
    return RT_OK;
}

} // namespace

extern "C" int rt_reproject_host(const float *src_fb, const float *src_sq, const int *src_count,
                                 const float *src_depth, const float *src_normal, const int32_t *src_triangle,
                                 Camera src_camera, const float *dst_depth, const float *dst_normal,
                                 const int32_t *dst_triangle, Camera dst_camera, int width, int height, float *dst_fb,
                                 float *dst_sq, int *dst_count, unsigned long long stats[3],
                                 const RtReprojectOptions *opt)
{
    RtRpParams prm;
    if (!rt_rp_resolve(opt, &prm)) {
        rt_set_error("rt_reproject_host: option out of range");
        return RT_E_INVALID;
    }
    const int rc = check_arguments("rt_reproject_host", src_fb, src_sq, src_count, src_depth, src_normal, dst_depth,
                                   dst_normal, width, height, dst_fb, dst_sq, dst_count);
    if (rc != RT_OK) return rc;
    const RtRpFrame src = {reinterpret_cast<const Vec3D *>(src_fb), src_sq, src_count, src_depth, src_normal,
                           src_triangle};
    reproject_frame<RT_SAMPLER_PINHOLE>(src, rt_rp_camera(src_camera), dst_depth, dst_normal, dst_triangle,
                                        rt_rp_camera(dst_camera), RtRpLens{0.0f, 0.0f, 0.0f, 0.0f}, width, height, prm,
                                        dst_fb, dst_sq, dst_count, stats);
    return RT_OK;
}

extern "C" int rt_reproject_sampler_host(const float *src_fb, const float *src_sq, const int *src_count,
                                         const float *src_depth, const float *src_normal, const int32_t *src_triangle,
                                         const RtSampler *src_sampler, const float *dst_depth, const float *dst_normal,
                                         const int32_t *dst_triangle, const RtSampler *dst_sampler, float *dst_fb,
                                         float *dst_sq, int *dst_count, unsigned long long stats[3],
                                         const RtReprojectOptions *opt)
{
    RtRpParams prm;
    if (!rt_rp_resolve(opt, &prm)) {
        rt_set_error("rt_reproject_sampler_host: option out of range");
        return RT_E_INVALID;
    }
    RtDevSampler ss, ds;
    if (const char *why = rt_rp_resolve_samplers(src_sampler, dst_sampler, &ss, &ds)) {
        rt_set_error("rt_reproject_sampler_host: %s", why);
        return RT_E_INVALID;
    }
    const int width = ds.width, height = ds.height;
    const int rc = check_arguments("rt_reproject_sampler_host", src_fb, src_sq, src_count, src_depth, src_normal,
                                   dst_depth, dst_normal, width, height, dst_fb, dst_sq, dst_count);
    if (rc != RT_OK) return rc;
    const RtRpFrame src = {reinterpret_cast<const Vec3D *>(src_fb), src_sq, src_count, src_depth, src_normal,
                           src_triangle};
    const RtRpLens lens = rt_rp_lens(ss, ds);
    switch (ds.kind) {
    case RT_SAMPLER_PINHOLE:
        reproject_frame<RT_SAMPLER_PINHOLE>(src, ss.cam, dst_depth, dst_normal, dst_triangle, ds.cam, lens, width,
                                            height, prm, dst_fb, dst_sq, dst_count, stats);
        break;
    case RT_SAMPLER_EQUIRECT:
        reproject_frame<RT_SAMPLER_EQUIRECT>(src, ss.cam, dst_depth, dst_normal, dst_triangle, ds.cam, lens, width,
                                             height, prm, dst_fb, dst_sq, dst_count, stats);
        break;
    case RT_SAMPLER_FISHEYE:
        reproject_frame<RT_SAMPLER_FISHEYE>(src, ss.cam, dst_depth, dst_normal, dst_triangle, ds.cam, lens, width,
                                            height, prm, dst_fb, dst_sq, dst_count, stats);
        break;
    default:
        reproject_frame<RT_SAMPLER_ORTHO>(src, ss.cam, dst_depth, dst_normal, dst_triangle, ds.cam, lens, width,
                                          height, prm, dst_fb, dst_sq, dst_count, stats);
        break;
    }
    return RT_OK;
}
