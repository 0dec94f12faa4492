// sampler_host_main.cpp — rt_sampler_rays_host (csrc/host/sampler_host.cpp) on
// hostile inputs, for a build with -fsanitize=address,undefined,
// float-cast-overflow (tests/test_samplers_sanitized.py): NaN and infinite
// cameras, FOVs, normals and points, 1x1 frames, pixel lists of INT32_MIN, -1,
// W*H and INT32_MAX.  The arrays are exactly n elements long, so a read or a
// write at index n is an error of the sanitizer's.
//
// Prints one line per case: "<rc> <kind> <WxH> <n> <rays with a non-finite
// component> <elements whose RNG state moved>".
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include <limits>
#include <vector>

#include "isaklm_rt.h"

void rt_set_error(const char *, ...) {}

static int run(const char *what, const RtSampler &s, long long n, bool centre)
{
    std::vector<uint32_t> rng((size_t)n);
    for (long long i = 0; i < n; ++i) rng[(size_t)i] = 0x9E3779B9u * (uint32_t)(i + 1);
    const std::vector<uint32_t> before = rng;
    std::vector<float> rays((size_t)n * 6, -1.0f);
    const int rc = rt_sampler_rays_host(&s, centre ? nullptr : rng.data(), n, rays.data());
    long long bad = 0, moved = 0;
    for (long long i = 0; i < n; ++i) {
        bool finite = true;
        for (int k = 0; k < 6; ++k) finite = finite && isfinite(rays[(size_t)i * 6 + k]);
        bad += !finite;
        moved += rng[(size_t)i] != before[(size_t)i];
    }
    printf("%d %s %dx%d %lld %lld %lld\n", rc, what, s.width, s.height, n, bad, moved);
    return rc;
}

int main()
{
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const Camera good = {{0.3f, 1.1f, -2.2f}, 0.4f, -0.15f, 1.2f, 0.03f};
    std::vector<Camera> cams = {good};
    const float hostile[] = {nan, inf, -inf, 3.0e38f, -1.0e30f};
    for (float v : hostile) {
        Camera c = good;
        c.yaw = v;
        cams.push_back(c);
        c = good;
        c.pitch = v;
        cams.push_back(c);
        c = good;
        c.FOV = v; // (FISHEYE rejects it: RT_E_INVALID, nothing computed)
        cams.push_back(c);
        c = good;
        c.aperture_radius = v;
        c.position.x = v;
        cams.push_back(c);
    }
    const int sizes[][2] = {{1, 1}, {3, 2}, {67, 45}};
    const char *names[] = {"pinhole", "equirect", "fisheye", "ortho"};
    int failures = 0;
    for (const Camera &cam : cams)
        for (int kind = RT_SAMPLER_PINHOLE; kind <= RT_SAMPLER_ORTHO; ++kind)
            for (const auto &sz : sizes) {
                const int W = sz[0], H = sz[1];
                RtSampler s = {kind, W, H, cam, 2.5f, nullptr, nullptr};
                const bool rejected = kind == RT_SAMPLER_FISHEYE && !(cam.FOV > 0.0f && cam.FOV <= 6.2831855f);
                for (int centre = 0; centre < 2; ++centre)
                    failures += run(names[kind], s, (long long)W * H, centre != 0) != (rejected ? RT_E_INVALID : RT_OK);
                // a pixel list with every kind of index outside the frame
                const std::vector<int32_t> pix = {0, INT32_MIN, -1, W * H, INT32_MAX, W * H - 1, W * H + 1, 0};
                s.pixels_device = pix.data();
                for (int centre = 0; centre < 2; ++centre)
                    failures += run(names[kind], s, (long long)pix.size(), centre != 0) != (rejected ? RT_E_INVALID : RT_OK);
            }
    // hemispheres: NaN, infinite, zero and unnormalised normals and points
    const float vals[] = {0.0f, -0.0f, 1.0f, -1.0f, nan, inf, -inf, 3.0e38f, 1.0e-30f};
    std::vector<float> pts;
    for (float a : vals)
        for (float b : vals)
            for (float c : vals) {
                const float p[6] = {c, a, b, a, b, c};
                pts.insert(pts.end(), p, p + 6);
            }
    RtSampler h = {RT_SAMPLER_HEMISPHERE, 0, 0, good, 0.0f, nullptr, pts.data()};
    failures += run("hemisphere", h, (long long)(pts.size() / 6), false) != RT_OK;
    failures += run("hemisphere", h, 1, false) != RT_OK;
    failures += run("hemisphere", h, 1, true) != RT_E_INVALID; // no centre ray
    return failures ? 1 : 0;
}
