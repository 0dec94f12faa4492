// convergence_host_main.cpp — rt_convergence_host (csrc/host/convergence_host.cpp)
// on hostile inputs, for a build with -fsanitize=address,undefined,
// float-cast-overflow (tests/test_convergence_sanitized.py): counts of
// INT32_MIN, -1, 0, 1, 2 and INT32_MAX, sums that are NaN, infinite, negative
// and huge, tolerances that are NaN, infinite, negative and 1e9, sizes 0, 1 and
// 257.  The arrays are exactly n elements long, so a read or a write at index n
// is an error of the sanitizer's.
//
// Prints one line per case: "<rc> <n> <min_samples> <tolerance index> <stats[0]>
// <stats[1]> <stats[2]> <stats[3]> <map entries that are +inf> <map entries
// that are NaN>", then one line "invalid <rc> ..." of the calls that must be
// rejected.
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include <limits>
#include <vector>

#include "isaklm_rt.h"

void rt_set_error(const char *, ...) {}

static const int kCounts[8] = {std::numeric_limits<int>::min(), -1, 0, 1, 2, 3, 1000, std::numeric_limits<int>::max()};

int main()
{
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float sums[7] = {0.0f, 0.75f, nan, inf, -inf, -2.5f, 3.0e38f};
    const float tolerances[7] = {0.05f, 0.3f, 0.0f, 1.0e9f, -1.0f, nan, inf};
    const int mins[5] = {0, 1, 4, 1001, std::numeric_limits<int>::max()};
    const long long sizes[3] = {0, 1, 257};
    for (long long n : sizes)
        for (int mi = 0; mi < 5; ++mi)
            for (int t = 0; t < 7; ++t) {
                const int m = mins[mi];
                // (exactly n elements: data() of an empty vector may be null, so n = 0 gets one element to point at)
                std::vector<float> rad((size_t)(n ? 3 * n : 3)), sq((size_t)(n ? n : 1)), err((size_t)(n ? n : 1), -1.0f);
                std::vector<int> cnt((size_t)(n ? n : 1));
                for (long long i = 0; i < n; ++i) {
                    cnt[(size_t)i] = kCounts[i % 8];
                    for (int k = 0; k < 3; ++k) rad[(size_t)(3 * i + k)] = sums[(i / 8 + k) % 7];
                    sq[(size_t)i] = sums[(i / 8 + 3 + i % 3) % 7];
                }
                if (n == 1) cnt[0] = kCounts[(mi + t) % 8];
                unsigned long long st[4] = {9, 9, 9, 9};
                const int rc = rt_convergence_host(rad.data(), sq.data(), cnt.data(), n, m, tolerances[t], err.data(), st);
                long long n_inf = 0, n_nan = 0;
                for (long long i = 0; i < n; ++i) {
                    n_inf += isinf(err[(size_t)i]) && err[(size_t)i] > 0;
                    n_nan += isnan(err[(size_t)i]);
                }
                printf("%d %lld %d %d %llu %llu %llu %llu %lld %lld\n", rc, n, m, t, st[0], st[1], st[2], st[3], n_inf, n_nan);
                // without the map and without stats
                if (rt_convergence_host(rad.data(), sq.data(), cnt.data(), n, m, tolerances[t], nullptr, nullptr) != rc)
                    return 3;
            }
    float f[4] = {0, 0, 0, 0};
    int c[1] = {0};
    unsigned long long st[4];
    printf("invalid %d %d %d %d %d %d %d\n", rt_convergence_host(nullptr, f, c, 1, 0, 0.05f, nullptr, st),
           rt_convergence_host(f, nullptr, c, 1, 0, 0.05f, nullptr, st),
           rt_convergence_host(f, f, nullptr, 1, 0, 0.05f, nullptr, st),
           rt_convergence_host(f, f, c, -1, 0, 0.05f, nullptr, st),
           rt_convergence_host(f, f, c, 1LL << 31, 0, 0.05f, nullptr, st),
           rt_convergence_host(f, f, c, 1, -1, 0.05f, nullptr, st),
           rt_convergence_host((const float *)((const char *)f + 2), f, c, 1, 0, 0.05f, nullptr, st));
    return 0;
}
