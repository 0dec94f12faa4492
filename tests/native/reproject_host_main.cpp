// reproject_host_main.cpp — rt_reproject_host (csrc/host/reproject_host.cpp)
// as a stand-alone program, for a run under AddressSanitizer + UBSan
// (tests/test_reproject_sanitized.py compiles both files with -fsanitize and
// runs this as a child process).  Seeded frames at 67 x 45, 3 x 2 and 1 x 1:
// depths that no geometry made (so projections land anywhere, far outside the
// frame included), counts of 0, misses, NaN / Inf / negative depths and sums,
// and cameras that are unmoved, moved, turned away, NaN and infinite — the
// float-to-int conversions of the tap positions are the point.  Every buffer
// is allocated at its exact size, so a read or write past an end is reported.
// Prints one line per run: "<status> <width>x<height> <camera> <non-finite
// outputs> <kept pixels> <checksum>".
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

int run(int w, int h, int which, Camera a, Camera b, const RtReprojectOptions *opt)
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
    const int rc = rt_reproject_host(fb.data(), sq.data(), count.data(), sd.data(), sn.data(), st.data(), a, dd.data(),
                                     dn.data(), which == 2 ? nullptr : dt.data(), b, w, h, ofb.data(), osq.data(),
                                     ocount.data(), stats, opt);
    size_t bad = 0;
    uint32_t sum = 0;
    for (size_t p = 0; p < n; ++p) {
        const float v[4] = {ofb[3 * p], ofb[3 * p + 1], ofb[3 * p + 2], osq[p]};
        for (float x : v) {
            if (!isfinite(x)) ++bad;
            uint32_t bits;
            memcpy(&bits, &x, 4);
            sum = sum * 31u + bits;
        }
        if (ocount[p] < 0 || ocount[p] > 5000) ++bad;
        sum = sum * 31u + (uint32_t)ocount[p];
    }
    printf("%d %dx%d %d %zu %llu %08x\n", rc, w, h, which, bad, stats[1], sum);
    return rc != 0 || bad != 0 || stats[0] != n;
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
    for (const auto &s : shapes)
        for (int c = 0; c < 6; ++c) {
            fails += run(s[0], s[1], c, base, cams[c], nullptr);
            fails += run(s[0], s[1], c, cams[c], base, &loose);
        }
    return fails ? 1 : 0;
}
