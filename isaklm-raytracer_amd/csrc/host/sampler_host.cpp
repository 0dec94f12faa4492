// sampler_host.cpp — rt_sampler_rays_host: rt_sampler_rays' arithmetic
// (sampler_math.h, the text the kernels compile) on host arrays.  The CPU tier
// of the samplers' tests, and a way to inspect a sampler's rays without a GPU:
// bit-identical to the GPU.  Depends on nothing but sampler_math.h.
#include "../sampler_math.h"

void rt_set_error(const char *fmt, ...);

extern "C" int rt_sampler_rays_host(const RtSampler *sampler, uint32_t *rng, long long n, float *rays)
{
    if (!rays) {
        rt_set_error("rt_sampler_rays_host: null rays");
        return RT_E_INVALID;
    }
    if (n < 0 || n > (1LL << 31) - 1) {
        rt_set_error("rt_sampler_rays_host: n = %lld out of [0, 2^31 - 1]", n);
        return RT_E_INVALID;
    }
    RtDevSampler smp;
    if (const char *why = rt_sampler_resolve(sampler, n, &smp)) {
        rt_set_error("rt_sampler_rays_host: %s", why);
        return RT_E_INVALID;
    }
    if (!rng && smp.kind == RT_SAMPLER_HEMISPHERE) {
        rt_set_error("rt_sampler_rays_host: a hemisphere sampler has no centre ray (null rng)");
        return RT_E_INVALID;
    }
#pragma omp parallel for schedule(static)
    for (long long e = 0; e < n; ++e) {
        Vec3D o, d;
        uint32_t st = 0;
        if (rng) {
            st = rng[e];
            rt_sampler_ray<false>(smp, (uint32_t)e, st, o, d);
            rng[e] = st;
        } else {
            rt_sampler_ray<true>(smp, (uint32_t)e, st, o, d);
        }
        float *r = rays + 6 * (size_t)e;
        r[0] = o.x; r[1] = o.y; r[2] = o.z;
        r[3] = d.x; r[4] = d.y; r[5] = d.z;
    }
    return RT_OK;
}
