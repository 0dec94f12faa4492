// convergence_host.cpp — rt_convergence_host: rt_convergence's arithmetic
// (convergence_math.h, the text the kernel compiles) on host arrays.  The CPU
// tier of the convergence tests, and the host side of a "render until
// converged" loop that already holds the frame: bit-identical to the GPU.
// Depends on nothing but convergence_math.h.
#include "../convergence_math.h"

void rt_set_error(const char *fmt, ...);

// the checks rt_convergence and rt_convergence_host share; nullptr = fine
const char *rt_cv_check(const void *radiance, const void *sq, const void *count, long long n, int min_samples,
                        const void *rel_error)
{
    if (!radiance || !sq || !count) return "null radiance, sq_luminance or sample_count";
    if (n < 0 || n > (1LL << 31) - 1) return "n out of range (0 .. 2^31 - 1)";
    if (((uintptr_t)radiance | (uintptr_t)sq | (uintptr_t)count | (uintptr_t)rel_error) & 3u)
        return "misaligned pointer (4 B)";
    if (min_samples < 0) return "min_samples < 0";
    return nullptr;
}

extern "C" int rt_convergence_host(const float *radiance, const float *sq_luminance, const int *sample_count,
                                   long long n, int min_samples, float tolerance, float *rel_error,
                                   unsigned long long stats[4])
{
    if (const char *why = rt_cv_check(radiance, sq_luminance, sample_count, n, min_samples, rel_error)) {
        rt_set_error("rt_convergence_host: %s", why);
        return RT_E_INVALID;
    }
    if (((uintptr_t)stats) & 7u) {
        rt_set_error("rt_convergence_host: stats is not 8-byte aligned");
        return RT_E_INVALID;
    }
    const RtCvParams prm = rt_cv_params(min_samples, tolerance);
    unsigned long long open = 0, below = 0, samples = 0;
#pragma omp parallel for schedule(static) reduction(+ : open, below, samples)
    for (long long e = 0; e < n; ++e) {
        const float *r = radiance + 3 * (size_t)e;
        const RtCvElement o = rt_cv_element(prm, rt_v3(r[0], r[1], r[2]), sq_luminance[e], sample_count[e]);
        if (rel_error) rel_error[e] = o.rel_error;
        open += o.open;
        below += o.below_min;
        samples += (unsigned long long)(long long)sample_count[e]; // (negative counts add modulo 2^64, as on the GPU)
    }
    if (stats) {
        stats[0] = (unsigned long long)n;
        stats[1] = open;
        stats[2] = below;
        stats[3] = samples;
    }
    return RT_OK;
}
