// denoise_host_main.cpp — rt_denoise_host (csrc/host/denoise_host.cpp) as a
// stand-alone program, for a run under AddressSanitizer + UBSan
// (tests/test_denoise_cpu.py compiles both files with -fsanitize and runs
// this as a child process).  Seeded synthetic frames at 37 x 29 (at spacing
// 16 most taps fall outside the frame on both sides) and 3 x 2, with counts
// of 0, misses and albedo channels below the demodulation floor, at 5 and 8
// levels and without demodulation; every buffer is allocated at its exact
// size, so a read or write past an end is reported.  Prints one line per
// run: "<status> <width>x<height> <non-finite outputs> <checksum>".
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "isaklm_rt.h"

void rt_set_error(const char *, ...) {}

namespace {

uint32_t g_state = 12345u;
float rnd() // [0, 1)
{
    g_state = g_state * 1664525u + 1013904223u;
    return (float)(g_state >> 8) * (1.0f / 16777216.0f);
}

int run(int w, int h, const RtDenoiseOptions *opt)
{
    const size_t n = (size_t)w * h;
    std::vector<float> fb(3 * n), sq(n), depth(n), normal(3 * n), albedo(3 * n), out(3 * n, -1.0f);
    std::vector<int> count(n);
    static const int counts[5] = {0, 1, 2, 7, 64};
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            const size_t p = (size_t)y * w + x;
            const int c = y == h / 2 ? 0 : counts[(int)(rnd() * 5.0f) % 5];
            count[p] = c;
            float lum = 0.0f;
            for (int k = 0; k < 3; ++k) {
                const float m = 2.0f * rnd();
                fb[3 * p + k] = m * (float)c;
                lum += m / 3.0f;
                albedo[3 * p + k] = rnd() < 0.2f ? 1.0f / 2048.0f : 0.05f + 0.9f * rnd();
            }
            sq[p] = (float)c * (lum * lum + rnd());
            const bool left = x < (w + 1) / 2;
            const bool miss = h >= 3 && y == (2 * h) / 3;
            depth[p] = miss ? INFINITY : (left ? 3.0f + 0.05f * x + 0.02f * y : 5.0f - 0.04f * x + 0.03f * y);
            const float nl[3] = {-0.6f, 0.0f, 0.8f}, nr[3] = {0.8f, 0.0f, 0.6f};
            for (int k = 0; k < 3; ++k) {
                normal[3 * p + k] = miss ? 0.0f : (left ? nl[k] : nr[k]);
                if (miss) albedo[3 * p + k] = 0.0f;
            }
        }
    const bool demodulate = !opt || opt->demodulate >= 0;
    const int rc = rt_denoise_host(fb.data(), sq.data(), count.data(), depth.data(), normal.data(),
                                   demodulate ? albedo.data() : nullptr, w, h, out.data(), opt);
    size_t bad = 0;
    uint32_t sum = 0;
    for (float v : out) {
        if (!isfinite(v)) ++bad;
        uint32_t b;
        memcpy(&b, &v, 4);
        sum = sum * 31u + b;
    }
    printf("%d %dx%d %zu %08x\n", rc, w, h, bad, sum);
    return rc != 0 || bad != 0;
}

} // namespace

int main()
{
    RtDenoiseOptions deep, plain;
    rt_default_denoise_options(&deep);
    deep.iterations = 8;
    rt_default_denoise_options(&plain);
    plain.demodulate = -1;
    int fails = 0;
    const int shapes[2][2] = {{37, 29}, {3, 2}};
    for (const auto &s : shapes) {
        fails += run(s[0], s[1], nullptr);
        fails += run(s[0], s[1], &deep);
        fails += run(s[0], s[1], &plain);
    }
    return fails ? 1 : 0;
}
