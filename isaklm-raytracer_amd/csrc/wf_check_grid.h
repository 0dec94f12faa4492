// The launch shape of wf_check, the run-time guard's KD re-trace (wavefront.hip;
// DESIGN.md §5 "Run-time guard").  Plain host C++, so that a CPU test can call it
// (tests/native/check_grid_check.cpp).
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
