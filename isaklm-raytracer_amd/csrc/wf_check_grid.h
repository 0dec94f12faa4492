// The sizes of the run-time guard (wavefront.hip; DESIGN.md §5 "Run-time guard"):
// the launch shape of wf_check, its KD re-trace, and the records a call may hold.
// Plain host C++, so that a CPU test can call it (tests/native/check_grid_check.cpp).
#pragma once
#include <cstdint>

// Blocks of `block` lanes for a call whose guard may record up to `want` rays
// (the host's upper estimate: the device's counter cannot be read at enqueue
// time) in a record buffer of `chk_cap` records per parity.
//
// * A chained call's check runs beside the next call's finisher or the
//   chain's drain: `min_blocks` (WF_CHECK_BLOCKS), whatever its place in the chain.
// * An unchained call's check runs alone on the chip after the finisher, and
//   the caller's synchronisation waits for it.  Each lock-step round of the
//   grid is one plain KD re-trace per lane, as long as its slowest ray, so the
//   call gets a lane per record: ceil(min(want, chk_cap) / block) blocks, at
//   least `min_blocks`.  Waves beyond the real record count leave at once.
// * Every lane's KD stack spills to spill[gtid + k * spill_threads]: the grid
//   may hold at most spill_threads lanes, i.e. spill_threads / block blocks.
//   That limit comes last: it holds whatever the other terms ask for.
static inline int wf_check_grid(bool chained, unsigned long long want, uint32_t chk_cap, int spill_threads, int block,
                                int min_blocks)
{
    const int limit = spill_threads / block;
    unsigned long long blocks = (unsigned long long)min_blocks;
    if (!chained) {
        const unsigned long long rec = want < chk_cap ? want : (unsigned long long)chk_cap;
        const unsigned long long b = (rec + (unsigned long long)block - 1ull) / (unsigned long long)block;
        blocks = b > blocks ? b : blocks;
    }
    return blocks > (unsigned long long)limit ? limit : (int)blocks;
}

// The records a whole call's guard is sized for: `want`, the host's estimate of the rays it records, and
// the return value, the record buffer's capacity per parity for it (0 and 0: the guard is off,
// check_mask 0xFFFFFFFF).  One ray in check_mask + 1 is recorded, of at most 8 rays per sample: deep
// paths go to wf_long, owed passes are few, so a small frame does not hold the 2 x max_cap maximum.
// Every ray recorded (check_mask 0, the tests' check_interval 1) leaves that average no slack: sized for
// the most a sample can trace before its hand-off at `depth` bounces, an extension and a shadow ray per
// bounce.  The capacity is a power of two from 2^16 up to max_cap (WF_CHECK_CAP): a frame beyond max_cap
// records per call can still drop some, which RtDeviations.check_dropped reports.
static inline uint32_t wf_check_records(unsigned long long slots, unsigned long long passes, uint32_t check_mask,
                                        int depth, uint32_t max_cap, unsigned long long *want)
{
    *want = 0;
    if (check_mask == 0xFFFFFFFFu) return 0;
    const unsigned long long per_sample = check_mask == 0u ? 2ull * (unsigned long long)depth + 2ull : 8ull;
    *want = slots * passes * per_sample / ((unsigned long long)check_mask + 1ull);
    uint32_t cap = 1u << 16;
    while (cap < *want && cap < max_cap) cap <<= 1;
    return cap;
}
