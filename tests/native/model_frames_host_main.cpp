// model_frames_host_main.cpp — rt_reproject_sampler_host and
// rt_denoise_sampler_host (csrc/host/reproject_host.cpp, denoise_host.cpp) as a
// stand-alone program, for a run under AddressSanitizer + UBSan
// (tests/test_model_frames_sanitized.py compiles the three files with
// -fsanitize and runs this as a child process).  The frames are
// reproject_host_main.cpp's kind: depths that no geometry made, counts of 0,
// misses, NaN / Inf / negative depths and sums; the cameras are unmoved, moved,
// turned away, NaN, infinite and 3e38 away, under all four image kinds — the
// models' projections (rt_atan2f, the fisheye's division, the wrapped tap
// columns) in front of the float-to-int conversions are the point.  The
// denoiser runs its periodic instantiation at widths 67, 5 and 1 (the taps
// alias).  Every buffer is allocated at its exact size.  Prints one line per
// run: "<status> <call> <kind> <width>x<height> <camera> <bad outputs> <kept>".
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "isaklm_rt.h"

void rt_set_error(const char *, ...) {}

namespace {

uint32_t g_state = 2463534242u;
float rnd() // [0, 1)
{
    g_state = g_state * 1664525u + 1013904223u;
    return (float)(g_state >> 8) * (1.0f / 16777216.0f);
}

float odd_value(float r, float v) // mostly v; sometimes a value a frame should never hold
{
    if (r < 0.03f) return NAN;
    if (r < 0.06f) return INFINITY;
    if (r < 0.08f) return -INFINITY;
    if (r < 0.10f) return -v;
    if (r < 0.12f) return 3.0e38f;
    return v;
}

RtSampler sampler(int kind, int w, int h, Camera cam)
{
    RtSampler s;
    memset(&s, 0, sizeof s);
    s.kind = kind;
    s.width = w;
    s.height = h;
    s.camera = cam;
    if (kind == RT_SAMPLER_FISHEYE) s.camera.FOV = 5.5f;
    s.ortho_half_width = 2.0f;
    return s;
}

int reproject(int kind, int w, int h, int which, Camera a, Camera b, const RtReprojectOptions *opt)
{
    const size_t n = (size_t)w * h;
    std::vector<float> fb(3 * n), sq(n), sd(n), sn(3 * n), dd(n), dn(3 * n), ofb(3 * n, -1.0f), osq(n, -1.0f);
    std::vector<int> count(n), ocount(n, -1);
    std::vector<int32_t> st(n), dt(n);
    static const int counts[6] = {0, 1, 2, 7, 64, 5000};
    for (size_t p = 0; p < n; ++p) {
        count[p] = counts[(int)(rnd() * 6.0f) % 6];
        for (int k = 0; k < 3; ++k) {
            fb[3 * p + k] = odd_value(rnd(), 2.0f * rnd() * (float)count[p]);
            sn[3 * p + k] = rnd() < 0.5f ? 0.0f : 1.0f;
            dn[3 * p + k] = sn[3 * p + k];
        }
        sq[p] = odd_value(rnd(), rnd() * (float)count[p]);
        sd[p] = odd_value(rnd(), 0.01f + 10.0f * rnd());
        dd[p] = which == 0 ? sd[p] : odd_value(rnd(), 0.01f + 10.0f * rnd());
        st[p] = (int32_t)(rnd() * 3.0f);
        dt[p] = st[p];
    }
    unsigned long long stats[3] = {0, 0, 0};
    const RtSampler sa = sampler(kind, w, h, a), sb = sampler(kind, w, h, b);
    const int rc = rt_reproject_sampler_host(fb.data(), sq.data(), count.data(), sd.data(), sn.data(), st.data(), &sa,
                                             dd.data(), dn.data(), which == 2 ? nullptr : dt.data(), &sb, ofb.data(),
                                             osq.data(), ocount.data(), stats, opt);
    size_t bad = 0;
    for (size_t p = 0; p < n; ++p) {
        const float v[4] = {ofb[3 * p], ofb[3 * p + 1], ofb[3 * p + 2], osq[p]};
        for (float x : v)
            if (!isfinite(x)) ++bad;
        if (ocount[p] < 0 || ocount[p] > 5000) ++bad;
    }
    printf("%d reproject %d %dx%d %d %zu %llu\n", rc, kind, w, h, which, bad, stats[1]);
    return rc != 0 || bad != 0 || stats[0] != n;
}

int denoise(int w, int h, int iterations)
{
    const size_t n = (size_t)w * h;
    std::vector<float> fb(3 * n), sq(n), depth(n), normal(3 * n), albedo(3 * n), out(3 * n, -1.0f);
    std::vector<int> count(n);
    static const int counts[5] = {0, 1, 2, 7, 64};
    for (size_t p = 0; p < n; ++p) {
        count[p] = counts[(int)(rnd() * 5.0f) % 5];
        const int axis = (int)(rnd() * 3.0f) % 3; // a unit normal along one axis
        for (int k = 0; k < 3; ++k) {
            fb[3 * p + k] = 2.0f * rnd() * (float)count[p];
            normal[3 * p + k] = k == axis ? 1.0f : 0.0f;
            albedo[3 * p + k] = rnd() < 0.2f ? 0.0f : rnd();
        }
        sq[p] = 4.0f * rnd() * (float)count[p];
        depth[p] = rnd() < 0.1f ? INFINITY : 0.01f + 10.0f * rnd();
        if (!(depth[p] < INFINITY)) normal[3 * p] = normal[3 * p + 1] = normal[3 * p + 2] = 0.0f;
    }
    Camera cam;
    memset(&cam, 0, sizeof cam);
    const RtSampler s = sampler(RT_SAMPLER_EQUIRECT, w, h, cam);
    RtDenoiseOptions o;
    rt_default_denoise_options(&o);
    o.iterations = iterations;
    const int rc = rt_denoise_sampler_host(fb.data(), sq.data(), count.data(), depth.data(), normal.data(),
                                           albedo.data(), &s, out.data(), &o);
    size_t bad = 0;
    for (float x : out)
        if (!isfinite(x) || x < 0.0f) ++bad;
    printf("%d denoise %d %dx%d %d %zu 0\n", rc, RT_SAMPLER_EQUIRECT, w, h, iterations, bad);
    return rc != 0 || bad != 0;
}

} // namespace

int main()
{
    const Camera base = {{0.3f, 1.5f, -2.0f}, 0.1f, -0.05f, 1.2f, 0.0f};
    Camera moved = base, away = base, nan_cam = base, inf_cam = base, huge = base;
    moved.position.x += 0.3f;
    moved.yaw += 0.05f;
    away.yaw += 3.14159265f;
    nan_cam.pitch = NAN;
    inf_cam.position.y = INFINITY;
    huge.position.z = -3.0e38f;
    const Camera cams[6] = {base, moved, away, nan_cam, inf_cam, huge};
    RtReprojectOptions loose;
    rt_default_reproject_options(&loose);
    loose.max_history = 1 << 20;
    loose.depth_tol = 3.0e38f;
    loose.normal_min = -0.999f;
    loose.match_triangle = -1;
    int fails = 0;
    const int shapes[3][2] = {{67, 45}, {3, 2}, {1, 1}};
    for (int kind = RT_SAMPLER_PINHOLE; kind <= RT_SAMPLER_ORTHO; ++kind)
        for (const auto &s : shapes)
            for (int c = 0; c < 6; ++c) {
                fails += reproject(kind, s[0], s[1], c, base, cams[c], nullptr);
                fails += reproject(kind, s[0], s[1], c, cams[c], base, &loose);
            }
    const int widths[3] = {67, 5, 1};
    for (int w : widths) {
        fails += denoise(w, 9, 5);
        fails += denoise(w, 1, 8);
    }
    return fails ? 1 : 0;
}
