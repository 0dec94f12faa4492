// wf_check's grid (csrc/wf_check_grid.h) over record estimates and spill areas:
// prints one line per case, "grid <chained> <want> <chk_cap> <spill_threads> -> <blocks>",
// for tests/test_guard_grid_host.py; exits 1 if a grid leaves its bounds.
#include <cstdio>
#include <cstdint>

#include "wf_check_grid.h"

int main()
{
    const int block = 256, min_blocks = 256;
    const uint32_t caps[] = {1u << 16, 1u << 20, 1u << 22};
    const int spills[] = {256 * block, 1024 * block, 1024 * block + 17, 4096 * block};
    int bad = 0;
    for (uint32_t cap : caps)
        for (int spill : spills) {
            const unsigned long long wants[] = {0ull,
                                                1ull,
                                                (unsigned long long)block,
                                                (unsigned long long)block + 1ull,
                                                (unsigned long long)min_blocks * block,
                                                (unsigned long long)min_blocks * block + 1ull,
                                                (unsigned long long)spill - 1ull,
                                                (unsigned long long)spill,
                                                (unsigned long long)spill + 1ull,
                                                (unsigned long long)cap,
                                                (unsigned long long)cap + 1ull,
                                                1ull << 40,
                                                ~0ull};
            for (unsigned long long want : wants)
                for (int chained = 0; chained < 2; ++chained) {
                    const int g = wf_check_grid(chained != 0, want, cap, spill, block, min_blocks);
                    printf("grid %d %llu %u %d -> %d\n", chained, want, cap, spill, g);
                    if (g < min_blocks || g > spill / block) ++bad;
                }
        }
    // a spill area smaller than the least grid (a device of fewer than 64 CUs): the area's limit wins
    const int small = wf_check_grid(false, 1ull << 20, 1u << 20, 100 * block, block, min_blocks);
    const int small_chained = wf_check_grid(true, 1ull << 20, 1u << 20, 100 * block, block, min_blocks);
    printf("small %d %d\n", small, small_chained);
    if (small != 100 || small_chained != 100) ++bad;
    // the record estimate and capacity a call's guard is sized for (wf_check_records), as launch_whole_now
    // calls it: "records <slots> <passes> <check_mask> <long_depth> -> <cap> <want>"
    const int deep_path = 64;        // RT_DEEP_PATH
    const uint32_t max_cap = 1u << 22; // WF_CHECK_CAP
    const struct { unsigned long long slots, passes; uint32_t mask; int long_depth; } calls[] = {
        {1920ull * 1080ull, 64, 4095u, 0},       // the bench frame
        {48ull * 27ull, 3, 0u, 0},               // the tests' check_interval 1, default hand-off depth
        {48ull * 27ull, 3, 0u, 16},              // ... and wf_long_depth 16
        {1920ull * 1080ull, 1024, 0u, 0},        // beyond the capacity's maximum
        {1920ull * 1080ull, 64, 0xFFFFFFFFu, 0}, // the guard off
    };
    for (const auto &c : calls) {
        unsigned long long want = ~0ull;
        const uint32_t cap = wf_check_records(c.slots, c.passes, c.mask, c.long_depth > 0 ? c.long_depth : deep_path,
                                              max_cap, &want);
        printf("records %llu %llu %u %d -> %u %llu\n", c.slots, c.passes, c.mask, c.long_depth, cap, want);
        if (cap > max_cap || (cap & (cap - 1u)) != 0u) ++bad;
    }
    printf("out of bounds %d\n", bad);
    return bad ? 1 : 0;
}
