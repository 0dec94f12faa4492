// denoise_math.h — the per-pixel arithmetic of rt_denoise, one text for the
// gfx950 kernels (denoise.hip) and the host tier (host/denoise_host.cpp).
//
// A variance-guided edge-avoiding a-trous filter over the G_Buffer's mean
// radiance, guided by the first-hit AOVs (DESIGN.md "Denoising" has the whole
// definition).  Every operation is a correctly rounded float32 operation
// (+ - * / sqrtf, compares) in the order written here — no expf / powf, no
// fused operations (every includer is built with -ffp-contract=off) — so the
// GPU, the host and a restatement in any IEEE float32 arithmetic give the
// same bits.  Maxima and minima are written as compares: fmaxf's choice
// between +0 and -0 is not fixed.
#pragma once

#include <math.h>

#include "rt_vecmath.h"

#define RT_DN_DEFAULT_ITERATIONS 5
#define RT_DN_DEFAULT_SIGMA_LUM 4.0f
#define RT_DN_DEFAULT_SIGMA_DEPTH 1.0f
#define RT_DN_DEFAULT_NORMAL_LOG2 7
#define RT_DN_MAX_ITERATIONS 8
#define RT_DN_MAX_NORMAL_LOG2 10
#define RT_DN_MIN_ALBEDO (1.0f / 1024.0f) // channels below it are not demodulated

// 16 bytes, 16-byte aligned: one vector load / store per record on the device
struct alignas(16) RtDn4 { float x, y, z, w; };

// the options with every default resolved
struct RtDnParams {
    int iterations;
    float sigma_lum, sigma_depth;
    int normal_log2;
    int demodulate; // 1 / 0
};

// RtDenoiseOptions (NULL = the defaults) -> RtDnParams; false: a value out of range
inline bool rt_dn_resolve(const RtDenoiseOptions *opt, RtDnParams *p)
{
    RtDenoiseOptions o = {0, 0.0f, 0.0f, 0, 0, nullptr};
    if (opt) o = *opt;
    p->iterations = o.iterations ? o.iterations : RT_DN_DEFAULT_ITERATIONS;
    p->sigma_lum = o.sigma_lum != 0.0f ? o.sigma_lum : RT_DN_DEFAULT_SIGMA_LUM;
    p->sigma_depth = o.sigma_depth != 0.0f ? o.sigma_depth : RT_DN_DEFAULT_SIGMA_DEPTH;
    p->normal_log2 = o.normal_log2 ? o.normal_log2 : RT_DN_DEFAULT_NORMAL_LOG2;
    p->demodulate = o.demodulate >= 0;
    if (p->iterations < 1 || p->iterations > RT_DN_MAX_ITERATIONS) return false;
    if (p->normal_log2 < 1 || p->normal_log2 > RT_DN_MAX_NORMAL_LOG2) return false;
    if (o.demodulate < -1 || o.demodulate > 1) return false;
    // negative, NaN and infinite sigmas (a NaN fails both compares)
    if (!(p->sigma_lum > 0.0f && p->sigma_lum <= 3.0e38f)) return false;
    if (!(p->sigma_depth > 0.0f && p->sigma_depth <= 3.0e38f)) return false;
    return true;
}

RT_HD float rt_dn_max0(float x) { return x > 0.0f ? x : 0.0f; }
RT_HD bool rt_dn_hit(float depth) { return depth < INFINITY; }
// the edge-stopping function: 1 at 0, ~x^-4 far out; a rational stand-in for exp(-x) that rounds the same everywhere
RT_HD float rt_dn_falloff(float x)
{
    const float r = 1.0f / (1.0f + x * x);
    return r * r;
}

// what the colour is divided by before filtering and multiplied by after it
RT_HD Vec3D rt_dn_demodulator(const float *albedo, size_t p, int demodulate)
{
    if (!demodulate) return rt_v3(1.0f, 1.0f, 1.0f);
    const float *a = albedo + 3 * p;
    return rt_v3(a[0] >= RT_DN_MIN_ALBEDO ? a[0] : 1.0f, a[1] >= RT_DN_MIN_ALBEDO ? a[1] : 1.0f,
                 a[2] >= RT_DN_MIN_ALBEDO ? a[2] : 1.0f);
}

// min(|z(+1) - z|, |z - z(-1)|) over the neighbours in the frame that hit; 0 without one
RT_HD float rt_dn_axis_slope(float z, bool has_next, float z_next, bool has_prev, float z_prev)
{
    const bool use_next = has_next && rt_dn_hit(z_next);
    const bool use_prev = has_prev && rt_dn_hit(z_prev);
    const float a = use_next ? fabsf(z_next - z) : 0.0f;
    const float b = use_prev ? fabsf(z - z_prev) : 0.0f;
    if (use_next && use_prev) return b < a ? b : a;
    return use_next ? a : b;
}

// x + dx on a periodic x axis (an equirectangular frame: longitude -pi and +pi are neighbours), for any dx
RT_HD int rt_dn_wrap(int xx, int width)
{
    xx %= width;
    return xx < 0 ? xx + width : xx;
}

// The prepare pass of pixel (x, y): the filter state (irradiance, variance of
// its mean luminance), the packed guides (normal, depth) and the depth slope.
// WRAP_X (rt_denoise_sampler on an EQUIRECT frame): every x neighbour is taken
// modulo width instead of clamped or dropped; rows never wrap (the poles are
// edges).  WRAP_X = false is rt_denoise's filter.
template <bool WRAP_X = false>
RT_HD void rt_dn_prepare_pixel(const Vec3D *fb, const float *sq, const int *count, const float *depth,
                               const float *normal, const float *albedo, int width, int height, int x, int y,
                               int demodulate, RtDn4 *state, RtDn4 *guide, float *slope)
{
    const size_t p = (size_t)y * width + x;
    const int n = count[p];
    const Vec3D f = fb[p];
    Vec3D c = rt_v3(0.0f, 0.0f, 0.0f); // (rows another shard owns have no samples)
    if (n > 0) c = f * (1.0f / (float)n);
    const Vec3D den = rt_dn_demodulator(albedo, p, demodulate);
    float var;
    if (n >= 2) { // adaptive_run's estimate (rt/path_tracing.cuh:352-376), of the mean
        const float tl = rt_luminance(f);
        var = rt_dn_max0((sq[p] - rt_square(tl) / (float)n) / (float)(n - 1)) / (float)n;
    } else { // one sample: standard deviation = mean
        var = rt_square(rt_luminance(c));
    }
    state->x = c.x / den.x;
    state->y = c.y / den.y;
    state->z = c.z / den.z;
    state->w = var / rt_square(rt_luminance(den));
    const float z = depth[p];
    guide->x = normal[3 * p];
    guide->y = normal[3 * p + 1];
    guide->z = normal[3 * p + 2];
    guide->w = z;
    float gx;
    if constexpr (WRAP_X) {
        const size_t row = (size_t)y * width;
        gx = rt_dn_axis_slope(z, true, depth[row + (x + 1 < width ? x + 1 : 0)], true,
                              depth[row + (x > 0 ? x - 1 : width - 1)]);
    } else {
        gx = rt_dn_axis_slope(z, x + 1 < width, x + 1 < width ? depth[p + 1] : 0.0f, x > 0,
                              x > 0 ? depth[p - 1] : 0.0f);
    }
    const float gy = rt_dn_axis_slope(z, y + 1 < height, y + 1 < height ? depth[p + width] : 0.0f, y > 0,
                                      y > 0 ? depth[p - width] : 0.0f);
    *slope = gx > gy ? gx : gy;
}

// One a-trous level at pixel (x, y), tap spacing `step`: the new state.  WRAP_X: as rt_dn_prepare_pixel — the
// tap order stays dy, then dx, from -2 to 2; taps that alias one pixel (2 * step >= width) are taken again.
template <bool WRAP_X = false>
RT_HD RtDn4 rt_dn_filter_pixel(const RtDn4 *state, const RtDn4 *guide, const float *slope, int width, int height,
                               int x, int y, int step, const RtDnParams &prm)
{
    const int p = y * width + x; // (width * height < 2^31)
    // the variance under a 3x3 Gaussian (1 2 1 / 2 4 2 / 1 2 1, over 16: every weight a power of two), rows
    // bottom to top, left to right, taps outside the frame clamped to its edge
    float vbar = 0.0f;
    for (int dy = -1; dy <= 1; ++dy) {
        int yy = y + dy;
        yy = yy < 0 ? 0 : (yy >= height ? height - 1 : yy);
        for (int dx = -1; dx <= 1; ++dx) {
            int xx = x + dx;
            if constexpr (WRAP_X) xx = xx < 0 ? width - 1 : (xx >= width ? 0 : xx);
            else xx = xx < 0 ? 0 : (xx >= width ? width - 1 : xx);
            const float g = (dx == 0 ? 0.5f : 0.25f) * (dy == 0 ? 0.5f : 0.25f);
            vbar += g * state[yy * width + xx].w;
        }
    }
    const float sd = prm.sigma_lum * sqrtf(rt_dn_max0(vbar)) + 1e-6f;

    const RtDn4 sp = state[p];
    const RtDn4 gp = guide[p];
    const float gz = slope[p];
    const bool hit_p = rt_dn_hit(gp.w);
    const float lum_p = rt_luminance(rt_v3(sp.x, sp.y, sp.z));
    const Vec3D n_p = rt_v3(gp.x, gp.y, gp.z);
    float sum_x = 0.0f, sum_y = 0.0f, sum_z = 0.0f, sum_v = 0.0f, sum_w = 0.0f;
    for (int dy = -2; dy <= 2; ++dy) {
        const int yy = y + step * dy;
        if (yy < 0 || yy >= height) continue;
        const int ay = dy < 0 ? -dy : dy;
        for (int dx = -2; dx <= 2; ++dx) {
            int xx = x + step * dx;
            if constexpr (WRAP_X) {
                xx = rt_dn_wrap(xx, width);
            } else {
                if (xx < 0 || xx >= width) continue;
            }
            const int ax = dx < 0 ? -dx : dx;
            const int q = yy * width + xx;
            const RtDn4 sq_ = state[q];
            const RtDn4 gq = guide[q];
            const float h = (ax == 0 ? 0.375f : (ax == 1 ? 0.25f : 0.0625f)) *
                            (ay == 0 ? 0.375f : (ay == 1 ? 0.25f : 0.0625f));
            const bool hit_q = rt_dn_hit(gq.w);
            const float wl = rt_dn_falloff(fabsf(lum_p - rt_luminance(rt_v3(sq_.x, sq_.y, sq_.z))) / sd);
            float w;
            if (hit_p != hit_q) {
                w = 0.0f;
            } else if (!hit_p) {
                w = h * wl;
            } else {
                float wn = rt_dn_max0(rt_dot(n_p, rt_v3(gq.x, gq.y, gq.z)));
                for (int k = 0; k < prm.normal_log2; ++k) wn = wn * wn;
                const float wz = rt_dn_falloff(fabsf(gp.w - gq.w) /
                                               (prm.sigma_depth * gz * (float)((ax + ay) * step) + 1e-4f * gp.w + 1e-30f));
                w = h * wn * wz * wl;
            }
            sum_x += w * sq_.x;
            sum_y += w * sq_.y;
            sum_z += w * sq_.z;
            sum_v += (w * w) * sq_.w;
            sum_w += w;
        }
    }
    // The centre tap's weight is 9/64 wn(p, p): positive for a unit normal.  A hit whose normal is shorter than
    // ~0.7 (a degenerate triangle's 0 among them) squares down to 0, and 0 / 0 would follow: such a pixel keeps
    // its state.
    if (!(sum_w > 0.0f)) return sp;
    RtDn4 out;
    out.x = sum_x / sum_w;
    out.y = sum_y / sum_w;
    out.z = sum_z / sum_w;
    out.w = sum_v / (sum_w * sum_w);
    return out;
}

// the last step: back to radiance
RT_HD Vec3D rt_dn_remodulate(const RtDn4 &s, Vec3D den) { return rt_v3(s.x * den.x, s.y * den.y, s.z * den.z); }
