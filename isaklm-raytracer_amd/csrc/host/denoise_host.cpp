// denoise_host.cpp — rt_denoise_host and rt_denoise_sampler_host: rt_denoise's
// arithmetic (denoise_math.h, the text the kernels compile) on host arrays.
// The CPU tier of the denoiser's tests, and the fall-back of an integrator
// without a GPU at hand: bit-identical to the GPU.  Depends on nothing but
// denoise_math.h and, for the sampler's checks, sampler_math.h.
#include <vector>

#include "../denoise_math.h"
#include "../sampler_math.h"

void rt_set_error(const char *fmt, ...);

extern "C" void rt_default_denoise_options(RtDenoiseOptions *o)
{
    if (!o) return;
    o->iterations = RT_DN_DEFAULT_ITERATIONS;
    o->sigma_lum = RT_DN_DEFAULT_SIGMA_LUM;
    o->sigma_depth = RT_DN_DEFAULT_SIGMA_DEPTH;
    o->normal_log2 = RT_DN_DEFAULT_NORMAL_LOG2;
    o->demodulate = 1;
    o->stream = nullptr;
}

namespace {

// the whole filter on checked arguments; WRAP_X: the x axis is periodic (denoise_math.h)
template <bool WRAP_X>
void denoise_frame(const float *fb, const float *sq, const int *count, const float *depth, const float *normal,
                   const float *albedo, int width, int height, float *rgb_out, const RtDnParams &prm)
{
    const size_t n = (size_t)width * height;
    std::vector<RtDn4> a(n), b(n), guide(n);
    std::vector<float> slope(n);
    const Vec3D *fb3 = reinterpret_cast<const Vec3D *>(fb);
#pragma omp parallel for schedule(static)
    for (int y = 0; y < height; ++y)
        for (int x = 0; x < width; ++x) {
            const size_t p = (size_t)y * width + x;
            rt_dn_prepare_pixel<WRAP_X>(fb3, sq, count, depth, normal, albedo, width, height, x, y, prm.demodulate,
                                        &a[p], &guide[p], &slope[p]);
        }
    RtDn4 *src = a.data(), *dst = b.data();
    for (int s = 0; s < prm.iterations; ++s) {
#pragma omp parallel for schedule(static)
        for (int y = 0; y < height; ++y)
            for (int x = 0; x < width; ++x)
                dst[(size_t)y * width + x] =
                    rt_dn_filter_pixel<WRAP_X>(src, guide.data(), slope.data(), width, height, x, y, 1 << s, prm);
        RtDn4 *t = src;
        src = dst;
        dst = t;
    }
#pragma omp parallel for schedule(static)
    for (int y = 0; y < height; ++y)
        for (int x = 0; x < width; ++x) {
            const size_t p = (size_t)y * width + x;
            const Vec3D c = rt_dn_remodulate(src[p], rt_dn_demodulator(albedo, p, prm.demodulate));
            rgb_out[3 * p] = c.x;
            rgb_out[3 * p + 1] = c.y;
            rgb_out[3 * p + 2] = c.z;
        }
}

// the options and the buffers both host calls check; who: the entry point's name
int check_arguments(const char *who, const float *fb, const float *sq, const int *count, const float *depth,
                    const float *normal, const float *albedo, const float *rgb_out, const RtDenoiseOptions *opt,
                    RtDnParams *prm)
{
    if (!rt_dn_resolve(opt, prm)) {
        rt_set_error("%s: option out of range", who);
        return RT_E_INVALID;
    }
    if (!fb || !sq || !count || !depth || !normal || !rgb_out || (prm->demodulate && !albedo)) {
        rt_set_error("%s: null buffer", who);
        return RT_E_INVALID;
    }
    return RT_OK;
}

} // namespace

extern "C" int rt_denoise_host(const float *fb, const float *sq, const int *count, const float *depth,
                               const float *normal, const float *albedo, int width, int height, float *rgb_out,
                               const RtDenoiseOptions *opt)
{
    RtDnParams prm;
    const int rc = check_arguments("rt_denoise_host", fb, sq, count, depth, normal, albedo, rgb_out, opt, &prm);
    if (rc != RT_OK) return rc;
    if (width < 1 || height < 1 || (long long)width * height > (1LL << 31) - 1) {
        rt_set_error("rt_denoise_host: bad frame size %d x %d", width, height);
        return RT_E_INVALID;
    }
    denoise_frame<false>(fb, sq, count, depth, normal, albedo, width, height, rgb_out, prm);
    return RT_OK;
}

extern "C" int rt_denoise_sampler_host(const float *fb, const float *sq, const int *count, const float *depth,
                                       const float *normal, const float *albedo, const RtSampler *sampler,
                                       float *rgb_out, const RtDenoiseOptions *opt)
{
    RtDnParams prm;
    const int rc = check_arguments("rt_denoise_sampler_host", fb, sq, count, depth, normal, albedo, rgb_out, opt, &prm);
    if (rc != RT_OK) return rc;
    RtDevSampler smp;
    if (const char *why = rt_sampler_resolve_frame(sampler, &smp)) {
        rt_set_error("rt_denoise_sampler_host: %s", why);
        return RT_E_INVALID;
    }
    if (smp.kind == RT_SAMPLER_EQUIRECT)
        denoise_frame<true>(fb, sq, count, depth, normal, albedo, smp.width, smp.height, rgb_out, prm);
    else
        denoise_frame<false>(fb, sq, count, depth, normal, albedo, smp.width, smp.height, rgb_out, prm);
    return RT_OK;
}
