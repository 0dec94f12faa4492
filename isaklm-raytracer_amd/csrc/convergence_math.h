// convergence_math.h — the per-element arithmetic of rt_convergence, one text
// for the gfx950 kernel (convergence.hip) and the host tier
// (host/convergence_host.cpp).
//
// The question is the adaptive test's (rt/path_tracing.cuh:352-376, rt_kernels.h
// adaptive_run): would the next pass run a sample on this element?  The
// operations are adaptive_run's, in its order: correctly rounded float32
// + - * / sqrtf and compares, no fused operations (every includer is built with
// -ffp-contract=off), so the GPU, the host and rt_render's own test give the
// same bits.  z_const = rt_adaptive_z(tolerance) is a host-side constant.
#pragma once

#include <math.h>

#include "rt_device.h"
#include "rt_vecmath.h"

struct RtCvParams {
    int min_samples;
    float tolerance;
    float z_const; // sqrtf(2) * erfinvf(1 - tolerance)
};

// the test's constants as rt_render makes them (host only; the tolerance is taken unchecked, as rt_render takes it)
inline RtCvParams rt_cv_params(int min_samples, float tolerance)
{
    RtCvParams p;
    p.min_samples = min_samples;
    p.tolerance = tolerance;
    p.z_const = rt_adaptive_z(tolerance);
    return p;
}

// the argument checks rt_convergence and rt_convergence_host share (host/convergence_host.cpp); nullptr = fine
const char *rt_cv_check(const void *radiance, const void *sq, const void *count, long long n, int min_samples,
                        const void *rel_error);

struct RtCvElement {
    bool open;       // adaptive_run would run a sample on the next pass
    bool below_min;  // count < min_samples
    float rel_error; // the diagnostic: iw / mean (open is never derived from it)
};

// One element.  A count below min_samples is open without arithmetic, as in adaptive_run; the interval is
// then computed only for count >= 2, where the map wants it — so no count - 1 is ever formed from a
// negative count (min_samples >= 0: a negative count is below it).
RT_HD RtCvElement rt_cv_element(const RtCvParams &p, Vec3D fb, float sq, int count)
{
    RtCvElement r;
    r.below_min = count < p.min_samples;
    r.open = r.below_min;
    r.rel_error = INFINITY;
    if (r.below_min && count < 2) return r;
    const float tl = rt_luminance(fb);
    const float mean = tl / (float)count;
    const float var = (sq - rt_square(tl) / (float)count) / (float)(count - 1);
    const float iw = p.z_const * sqrtf(var / (float)count);
    if (!r.below_min) r.open = iw > mean * p.tolerance;
    if (count >= 2) r.rel_error = iw > 0.0f ? iw / mean : 0.0f;
    return r;
}
