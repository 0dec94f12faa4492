// wf_state.h — the wavefront kernels' tuning constants, the pixel ownership word, WfState and the
// queue / hand-off publish helpers.
// A part of wavefront.hip's translation unit (included there, once, in the order wf_state.h,
// wf_queue_kernels.h, wf_shade.h, wf_finish_kernels.h, wf_long.h): not for use elsewhere.
#pragma once

#define WF_BLOCK 256
#ifndef WF_TBLOCK
#define WF_TBLOCK 256 // threads per block of the queue kernels (wf_trace_coop, wf_shade)
#endif
// tgrid * WF_TBLOCK == grid * WF_BLOCK threads: the spill area (sized for
// grid * WF_BLOCK threads, indexed by the global thread id) must cover them
static_assert(WF_BLOCK % WF_TBLOCK == 0 && WF_TBLOCK % 64 == 0, "WF_TBLOCK must divide WF_BLOCK in whole waves");
// wave priorities beside the other pipelines' trace waves (A/B, 4 rounds:
// -1 % call time together): a pipeline's shade launch and the tail of its
// trace launch are on its critical path, the other launches' bulk is not
#ifndef WF_SHADE_PRIO
#define WF_SHADE_PRIO 3
#endif
// wf_shade runs in the slots its pipeline's trace launch just left, beside
// the other pipelines' trace waves (80 VGPRs each): at the same footprint
// (6 waves/SIMD, the rest of its ~126 VGPRs spilled) its waves fit those
// holes.  Measured (room2m 1080p, 256 passes/call, 3 rounds, s per call):
// 13.83 at 126 VGPRs, 13.58 at 96, 13.21 at 80, 13.21 at 72, 13.31 at 64
// (and 13.60 for the earlier 102-VGPR build that kept its path state in scratch)
#ifndef WF_SHADE_WAVES
#define WF_SHADE_WAVES 6
#endif
// wf_long, too, runs beside the pipelines' trace waves: at their footprint
// (80 VGPRs, ~85 spilled) its waves fit the slots a trace block leaves.
// Measured (as WF_SHADE_WAVES): 13.16 s at 126 VGPRs, 13.16 at 128 (4
// waves), 12.87 at 80, 12.86 at 72, 12.92 at 64
// Whole-call mode (the default render): a wf_long block takes the slot of a
// finisher block — 4 waves, one per SIMD, beside 3 finisher waves of 128 VGPRs
// each —, so 128 VGPRs cost it no residency and halve its spills (200 -> 101
// with the wave-wide bounded bounce): 13.3-14.0 vs 14.4-15.6 us per deep
// bounce alone (room_small sphere) and 18.0-18.8 vs 20.3-21.5 beside a running
// finisher (room2m), a lone 256-pass room2m call's last deep sample ending at
// 888 vs 981 ms (profiles/deep_bounded/).
#ifndef WF_LONG_WAVES
#define WF_LONG_WAVES 4
#endif
#ifndef WF_LONG_PRIO
// wf_long wave priority: a deep path's bounce chain is the call's critical
// path, and in the whole-call mode its wave shares a CU with ~24 finisher
// waves; s_setprio 3 wins it the issue arbitration.  Per 256-pass room2m call
// (5 calls x 2 rounds, tools/gpu_ab_libs5.sh): 6.93 / 6.96 s vs 7.34 / 7.80 s
// for 5 calls at priority 0 (-5.6 % / -11 %)
#define WF_LONG_PRIO 3
#endif
#ifndef WF_FIN_LINGER
#define WF_FIN_LINGER 100000000ull // s_memrealtime ticks (100 MHz): 1 s
#endif
#ifndef WF_FIN_LINGER_WAVES
#define WF_FIN_LINGER_WAVES 256u // finisher waves that linger for returned pixels
#endif
#ifndef WF_HEAVY_FIRST
#define WF_HEAVY_FIRST 1 // whole-call finisher: pixels whose paths went to wf_long before start the call
#endif
#define WF_HEAVY_BLOCKS 256
#ifndef WF_HEAVY_SPLIT
#define WF_HEAVY_SPLIT 4 // hand-offs that put a pixel in the first class (1: one class)
#endif
#ifndef WF_FIN_QUIET_TRIPS
#define WF_FIN_QUIET_TRIPS 4096u // ... while wf_long ran a path within this many of their idle loop trips
#endif
#define WF_FIN_LINGER_TRIPS 1000000u // ... and for at most this many idle loop trips in all (a bound that holds
                                     // where s_memrealtime stands still: rocprofv3 counter collection)
#ifndef WF_FIN_OCC
#define WF_FIN_OCC 1 // wf_finish_coop occupancy floor (1: the compiler's choice, 2 waves/SIMD; 3: no change)
#endif
#ifndef WF_TAIL_PRIO
#define WF_TAIL_PRIO 2
#endif
#ifndef WF_LDS_STACK
#define WF_LDS_STACK 8  // stack entries in LDS; deeper ones spill to HBM (rare)
#endif
#ifndef WF_TRACE_WAVES
#define WF_TRACE_WAVES 6 // wf_trace_coop occupancy target (blocks of 4 waves per CU = waves per SIMD)
#endif
#ifndef WF_BVH_LDS
#define WF_BVH_LDS 10   // wf_finish_bvh: stack entries in LDS (BVH query and KD descent share the
                        // stack; deeper entries go to the HBM spill area).  10 (34.8 KB per block: 4 finisher blocks
                        // and a wf_long block fit a CU's 160 KB) vs 8 / 9: 745-748 vs 735-738 / 735-742 Msamples/s
                        // (round 6, profiles/r06/ab/ ab19); 12 left no room for the wf_long block (-9 %)
#endif
#ifndef WF_CHECK_BLOCKS
#define WF_CHECK_BLOCKS 256 // wf_check's grid for a chained call (it runs beside the next call's finisher or the
                            // drain), and the least an unchained call gets: alone on the chip, that one's grid
                            // follows its records up to the spill area's lanes (wf_check_grid.h)
#endif
#ifndef WF_BVH_BUDGET
#define WF_BVH_BUDGET 14 // wf_finish_bvh: bodies — node steps and leaf visits, each for whichever lanes hold one — the
                         // WAVE executes per loop trip before every unfinished s_min query parks (bvh_trace.h
                         // bvh4_query_budget; it replaced WF_BVH_PARK = 6, a cap on each lane's own node steps under
                         // which the wave ran ~21 bodies per trip; 12 / 14 / 18: profiles/query_budget/)
#endif
#define WF_DEBUG_BUDGET1 2 // WfState.chk_fault bit (RtOptions.debug RT_DEBUG_BUDGET1): the counting finisher's budget is 1
#ifndef WF_KD_PEND_MIN
#define WF_KD_PEND_MIN 4 // wf_finish_bvh: lanes of a wave waiting for their KD descent (rays the T* certificate does
                         // not cover, RT_PARK_KD) before a loop trip runs them; fewer wait — unless the wave has
                         // nothing else to do (1 / 4 / 8 / 16 / 64 = 770-777 / 782-785 / 763-772 / 753-754 / 319-321
                         // Msamples/s, profiles/kd_cert/pend_min_sweep.txt; 8 shipped with the certificate, 4 since
                         // the GPU suite ran on it: profiles/guard_refit/)
#endif
#ifndef WF_FIN_BVH_WAVES
#define WF_FIN_BVH_WAVES 4 // wf_finish_bvh occupancy target: 4 waves/SIMD (128 VGPRs, 29 spilled) run the bench at
                           // 5's rate (566.8-572.2 vs 562.8-573.1 Msamples/s, round 6) with a third of its HBM traffic
                           // for spills: 107 vs 324 GB written and 908 vs 1,350 GB fetched per 256-pass call
                           // (profiles/r06/bench_w4_pmc.json); 6: -9 %.  (Round 5 kept 5 because 4's counter passes
                           // hung: that was wf_long's start race, fixed in round 6, not the occupancy)
#endif
// (chained calls' finishers run one after the other on pipeline 0: a kernel boundary between calls,
// which a pixel's state crosses for free.  The round-5 variants — a finisher going on with the next
// issued call, finishers alternating between two streams — measured slower, one of them inexact,
// and are gone: DESIGN.md §6 keeps their A/B records)
#ifndef WF_NEE_LDS
#define WF_NEE_LDS 1 // wf_finish_bvh keeps a NEE set-up's state in LDS (PathRegsL), not in registers: at 4 waves/SIMD
                     // 8 VGPRs spilled instead of 30, 64 instead of 107 GB written per 256-pass call, the bench
                     // unchanged (569.5 vs 569.3; profiles/r06/bench_nee_lds_pmc.json)
#endif
#ifndef WF_FIN_SMALL_WAVES
#define WF_FIN_SMALL_WAVES 3 // frames of at most this many finisher waves per SIMD take the unspilled build (151 VGPRs: 3 waves)
#endif
// per-thread spill entries: the deeper of the KD stack (past WF_LDS_STACK) and the BVH stack (past WF_BVH_LDS)
#define WF_SPILL_ENTRIES \
    ((RT_STACK_DEPTH - WF_LDS_STACK) > (RT_BVH_STACK - WF_BVH_LDS) ? (RT_STACK_DEPTH - WF_LDS_STACK) \
                                                                    : (RT_BVH_STACK - WF_BVH_LDS))
#define WF_TAIL_DEFAULT 65536u       // RtOptions.wf_tail
#define WF_FINISH_WAVES_DEFAULT 2048u // RtOptions.wf_finish_waves
#define WF_FINISH_WAVES_SMALL 512u    // ... for trees below WF_FIN_WIDE_MIN_ENTRIES leaf entries
#define WF_DESCENT_CAP_DEFAULT 5      // RtOptions.wf_descent_cap
#define WF_POSTPONE_DEFAULT 20        // RtOptions.wf_postpone
#define WF_TIMELINE_LAUNCHES 4096     // debug timeline: 3 u64 per trace launch in RtOptions.wave_times_device
#define WF_WIDE_TAIL_LANES 32         // RtOptions.wf_wide > 0
#define WF_FIN_WIDE_MIN_ENTRIES (1 << 18) // finisher: multi-ray wide tracing only for trees with this many leaf entries
#define WF_MAX_PIPES 6                // concurrent pipelines (RtOptions.wf_pipelines); more than 3 need GPU_MAX_HW_QUEUES > 4
#define WF_PIPES_DEFAULT 3
#ifndef WF_LONG_DEPTH_DEFAULT
#define WF_LONG_DEPTH_DEFAULT 64      // RtOptions.wf_long_depth: paths deeper than this go to wf_long
#endif
#define WF_LONG_DEPTH_MIN 16          // ... smaller values are raised to this (profiles/r05/small_calls/long_depth_sweep)
#define WF_COALESCE_DEFAULT 256       // RtOptions.coalesce_passes: chained calls are coalesced up to this many passes
#ifndef WF_LONG_BLOCKS
#define WF_LONG_BLOCKS 64 // wf_long grid (4 waves each, one path per wave at a time)
#endif
// Cross-kernel waits (finisher <-> wf_long).  No kernel may wait for work of
// a kernel that is not resident: under rocprofv3 counter collection the
// dispatches are serialised (either kernel may run first, alone), and a shared
// chip may delay either one.  So every such wait is bounded by a count of the
// waiting loop's trips — s_memrealtime stands still under counter collection
// (ae07d5e), so the clock bounds below are a second, faster exit, never the
// only one — and a bound that expires leaves the protocol in a state the
// other side completes on its own:
//  * wf_long waits for its call's finisher only once a finisher wave has
//    started (WF_FIN_STARTED).  Before that it waits at most
//    WF_LONG_START_TRIPS idle trips, then CLOSES the hand-off ring
//    (WF_LONG_CLOSED in the reserved counter, set only while every reserved
//    entry is claimed) and leaves: the finisher's hand-offs then fail and its
//    lanes run their deep paths to the end themselves (the same shade_step
//    sequence: bit-identical).  The ring stays closed until the next call
//    that does not continue a chain resets it (RT_DEV_LONG_CLOSED counts it);
//  * a finisher lingers for pixels out in wf_long at most WF_FIN_QUIET_TRIPS
//    trips while no wf_long wave runs a path, and at most st.linger ticks;
//  * a finisher claims a return wf_long reserved only while wf_long is
//    resident (it reserves while running); its wait for the entry's
//    publication is bounded by WF_SPIN_TRIPS (expired: the pixel is left out,
//    found by wf_verify, RT_E_INCOMPLETE);
//  * the safety nets of wf_long's claim loop, never reached by a working
//    protocol: an entry reserved but never published (WF_LONG_PUBLISH_TRIPS /
//    _WAIT) and nothing left that could bring work (WF_LONG_IDLE_TRIPS /
//    WF_LONG_IDLE).  A net exit with entries unclaimed strands pixels instead
//    of hanging the GPU — counted (RT_DEV_LONG_QUIT), found by the join's
//    wf_verify and reported.
// (A trip of these loops is an s_sleep plus 2-4 L2 atomics: ~1-2 us.)
#define WF_FIN_STARTED 0x80000000u        // fin_live: a finisher wave of the call has started
#define WF_LONG_CLOSED 0x80000000u        // long_ctr[0]: the ring takes no more hand-offs
#define WF_LONG_START_TRIPS 20000u        // idle trips before wf_long closes the ring on an unstarted finisher
#define WF_LONG_IDLE 200000000ull         // 2 s idle with nothing that could still bring work
#define WF_LONG_IDLE_TRIPS 2000000u       // ... or this many trips
#define WF_LONG_PUBLISH_WAIT 100000000ull // 1 s on one reserved, unpublished entry (publication is ~1 us)
#define WF_LONG_PUBLISH_TRIPS 1000000u    // ... or this many trips
#define WF_SPIN_TRIPS (1u << 24)          // a finisher lane's wait for a reserved return's publication
// an idle persistent wf_long wave of an open chain stays until no entry has
// been reserved (for any wave) for this long (50 ms, or WF_LONG_CHAIN_TRIPS
// trips) AND no wave runs a path: the next calls' deep paths
// (WfState.chain_flag).  The grid leaves as a whole — one whose idle waves
// left while a few ran 10^4-bounce samples on (a call's tail can go 50 ms
// without a hand-off) served the next calls with those few waves, its
// stream-queued successor blocked behind them.
#define WF_LONG_CHAIN_IDLE 5000000ull
#define WF_LONG_CHAIN_TRIPS 50000u
// RtOptions.check_interval: 1 ray in this many re-traced by the KD traversal
// (a KD re-trace costs ~50 bounded queries: 1024 took 4 % of a 256-pass
// room2m call, 4096 ~1 %, and still checks ~2M rays in the 20-step bench)
#define WF_CHECK_INTERVAL_DEFAULT 4096u
#define WF_CHECK_CAP (1u << 22)         // cross-check records per launch (more are dropped: RT_DEV_CHK_DROP;
                                        // a chained launch may run several calls' pixels)
// per-pixel ownership word (WfState.pxo) of the whole-call render: a pixel is
// BUSY while a finisher lane runs its passes and OUT while wf_long holds it
// (handed over, or in the return ring), until a finisher lane takes it back or
// wf_long finishes it.  A call that finds its pixel held adds its passes to
// the low bits (owed) and moves on; the holder runs them, in the pixel's order,
// before it lets go.  Free: 0, or REL when the last holder may run concurrently
// with the next one (a chained finisher, wf_long): its stores were released
// before the word said so, and the next claimer acquires first.
#define RT_PX_OUT 0x80000000u
#define RT_PX_REL 0x40000000u
#define RT_PX_LONGDONE RT_PX_REL
#define RT_PX_BUSY 0x20000000u
#define RT_PX_PASSES 0x1FFFFFFFu

struct WfState {
    int *passes_left;
    uint32_t *flags;   // bit0 shadow, bit1 inside, bits 2..4 prev_type, bit5 dual, bit6 ext_live, bits 8.. depth
    Vec3D *T, *L, *cont, *snorm, *rp;
    Vec3D *ro;         // origin of the path's pending ray(s); cont = the pending extension direction
    uint32_t *e_sh, *e_ext; // queue entries of the path's pending shadow / extension ray
    int *light;
    uint32_t *q_slot[2]; // path lists: the pixels (slots) with rays in ray queue q
    RtF4 *q_ray[2];    // ray queues, 2 RtF4 per entry: {o.xyz, -}, {d.xyz, -}
    RtF4 *hits;        // per ray-queue entry: {tri bits, bx, by, bz}
    uint32_t *counts;  // [0], [1]: ray queue sizes; [2], [3]: fetch cursors; [4] finisher fetch; [6], [7]: path list sizes
    uint2 *spill;      // traversal stack spill
    int spill_threads;
    // long-path hand-off (wf_long): a path deeper than long_depth leaves its
    // pipeline for the concurrently running wf_long kernel through a ring of
    // long_cap entries: entry e (counted from the last reset) lives at e %
    // long_cap, published as long_ent = (e + 1) << 32 | slot after its ray
    uint32_t *long_ctr;   // [0] entries reserved (| WF_LONG_CLOSED), [1] entries claimed, [3] paths running in wf_long
    unsigned long long *long_ent;
    RtF4 *long_ray;       // 2 per ring slot
    int long_depth;       // 0 = off
    uint32_t long_cap;    // ring slots (the pixels)
    // whole-call finisher (bounded traversal): wf_long runs a handed-over path
    // only to the end of its SAMPLE and returns the pixel through this ring to
    // the finishers, whose lanes run its remaining passes
    int long_return;
    unsigned long long *ret_ring; // entry e at e % long_cap: (e + 1) << 32 | slot once published
    unsigned long long *long_log; // debug (RT_DEBUG_LONG_LOG): [0] call start, then per claim {claim, end, bounces, slot}
    // ret_ctr: u64 [0] = finisher waves alive << 32 | returns reserved (wf_long
    // reserves only while a finisher wave is alive; a wave leaves only when
    // every reserved return is claimed: no pixel is stranded.  The finisher
    // never waits for a wf_long that is not resident: returns are reserved by
    // a running wf_long wave, and lingering is bounded — see the cross-kernel
    // waits above);
    // u32 [2] = returns claimed, u32 [3] = pixels out (handed to wf_long, not
    // yet returned or done): an idle finisher wave lingers (s_sleep) while
    // pixels are out — for at most `linger` ticks (0 for chained calls, whose
    // successor takes the returns), so that it never depends on wf_long
    uint32_t *ret_ctr;
    unsigned long long linger;
    // per pixel: RT_PX_OUT / RT_PX_BUSY | passes owed by later chained calls, RT_PX_REL, or 0
    uint32_t *pxo;
    // heavy pixels first (whole-call finisher): a pixel whose path went to wf_long is marked
    // (heavy); before each call wf_heavy_list lists the marked pixels (heavy_list, count
    // heavy_n) and tags them with the call (listed): the finisher's first entries are those
    // pixels, and its tile entries skip a pixel listed for this call.  heavy_list == nullptr:
    // no list (the tiles only)
    uint8_t *heavy;
    uint32_t *listed, *heavy_list, *heavy_n;
    // the whole-call finisher takes this call's pixels itself (no wf_start, no path list): fresh = 1
    int fresh;
    uint32_t fresh_n; // (fresh) entries: 256 per 16x16-pixel tile (fresh_pixel); 0 for a chain's drain
    unsigned long long *span; // RtOptions.profile: {first wave start, last wave end} (s_memrealtime)
    uint32_t call_id; // this launch's call (heavy-pixel list tags)
    // the persistent wf_long's producers: the host sets the word to the finisher's wave count;
    // each finisher wave sets WF_FIN_STARTED when it starts and subtracts 1 once past its last
    // hand-off (nullptr: wf_long runs in host-kicked slices).  wf_long waits for producers only
    // once one has started: a finisher not yet dispatched (counter collection serialises
    // dispatches) is never waited for
    uint32_t *fin_live;
    // 1 while a chain of calls is open (set by chained calls, cleared by its
    // drain): an idle persistent wf_long wave then stays up to WF_LONG_CHAIN_IDLE
    // for the later calls' deep paths instead of leaving at its first idle
    // moment (which left the next calls' entries to the few waves still busy,
    // the stream-queued successor blocked behind them).  Bounded: the drain's
    // clear may sit behind this very wf_long when streams share a hardware queue.
    uint32_t *chain_flag;
    // run-time exactness guard of the bounded traversal: the finisher records
    // every ray whose hash of (pixel, pass, depth, kind) hits chk_mask (3 RtF4:
    // {o, hit bits}, {d, bx}, {by, bz, -, -}); wf_check re-traces them with the
    // plain KD traversal (nullptr: off)
    RtF4 *chk;
    uint32_t *chk_ctr;
    uint32_t chk_mask;
    uint32_t chk_cap; // records per parity (more are dropped: RT_DEV_CHK_DROP)
    int chk_fault; // (bit 0: RT_DEBUG_CHECK_FAULT, tests: record a wrong result for every checked ray; WF_DEBUG_BUDGET1)
    int debug_quit; // (RT_DEBUG_LONG_QUIT, tests: wf_long leaves at once, as by its safety net)
    // wf_long's bounded bounces (whole-call mode): the wave-wide s_min query and the wave-run bounded KD
    // traversal (wide_bvh.h).  0: off (the wide KD traversal), 1: on, 2: on with list capacity 1
    // (RT_DEBUG_WIDE_CAP1, tests: every query overflows and the ray takes the wide KD traversal)
    int long_wide;
};

// RT_COLD_ARGS: what a loop trip of wf_finish_bvh does not read leaves the registers.  A kernel's by-value
// arguments are loaded into scalar registers at its entry and stay live to their last use: the finisher's ~190
// argument dwords against ~100 registers put 200 of them into vector-register lanes (v_writelane / v_readlane
// around every use, three VGPRs held for them while 12 others went to scratch).  The fields only rare paths
// read — the hand-off and return rings and their counters, the heavy list, the ownership words, the path
// state arrays of store_regs / first_ray, the guard's record buffer, span and the debug fields — are now read
// where they are used, from the kernel's own argument block: the kernarg segment is device memory the
// dispatch wrote for this launch, read-only to the kernel, and its address is wave-uniform, so each read is
// one scalar load through the scalar cache.  No second copy of the state exists and the host does nothing
// new.  wf_cold_state() hands out the WfState argument in place; its address passes through an empty asm
// so that the compiler cannot move the loads back to the kernel's entry.  For the kernels whose arguments
// start (RtDevScene, RtDevFrame, RtDevCamera, WfState): wf_finish_bvh and wf_long (the offset is checked
// against the code object's own argument table in tests/test_fin_resources.py).
#ifndef RT_COLD_ARGS
#define RT_COLD_ARGS 1 // 0 (a HIP compile flag, for A/B): every field from the by-value argument
                       // (NOT the build before the switch: the source around the reads — the cs / cf locals, ret_word
                       // recomputed where it is used — allocates differently even with the macros the identity:
                       // 207 SGPR / 23 VGPR spills in wf_finish_bvh<false, 4> against 200 / 12 before.  A bisect
                       // with the switch overstates the gain; compare with the commit before it, as DESIGN §9 does)
#endif
constexpr size_t wf_align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
constexpr size_t WF_KERNARG_FRAME = wf_align_up(sizeof(RtDevScene), alignof(RtDevFrame));
constexpr size_t WF_KERNARG_CAMERA = wf_align_up(WF_KERNARG_FRAME + sizeof(RtDevFrame), alignof(RtDevCamera));
constexpr size_t WF_KERNARG_STATE = wf_align_up(WF_KERNARG_CAMERA + sizeof(RtDevCamera), alignof(WfState));
// (the values tests/test_fin_resources.py finds in the built kernels' argument tables)
static_assert(WF_KERNARG_FRAME == 248 && WF_KERNARG_CAMERA == 360 && WF_KERNARG_STATE == 416 && sizeof(WfState) == 344,
              "kernarg layout of (RtDevScene, RtDevFrame, RtDevCamera, WfState, ...): update tests/test_fin_resources.py");
#if RT_COLD_ARGS && defined(__HIP_DEVICE_COMPILE__)
// The empty `asm volatile` with "+s" is all that keeps the loads at their use: it makes the pointer opaque and
// cannot itself be hoisted or merged.  A compiler that saw through it would load the fields at the entry again
// and the spills would return — nothing would break, and tests/test_fin_resources.py's bound on sgpr_spill_count
// (the value this build reaches) is what would fail: that test failing after a compiler upgrade means this.
typedef const RT_CONST WfState WfCold;
__device__ __forceinline__ WfCold &wf_cold_state()
{
    const RT_CONST char *k = (const RT_CONST char *)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(k));
    return *reinterpret_cast<WfCold *>(k + WF_KERNARG_STATE);
}
// (the camera, read once per sample start: a copy in registers for that block only)
__device__ __forceinline__ RtDevCamera wf_cold_camera()
{
    const RT_CONST char *k = (const RT_CONST char *)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(k));
    return *reinterpret_cast<const RT_CONST RtDevCamera *>(k + WF_KERNARG_CAMERA);
}
// (the frame, for the blocks that start a sample, claim a pixel or shade: live inside such a block, not across
// the traversal loops; the compiler loads only the fields the block reads)
__device__ __forceinline__ RtDevFrame wf_cold_frame()
{
    const RT_CONST char *k = (const RT_CONST char *)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(k));
    return *reinterpret_cast<const RT_CONST RtDevFrame *>(k + WF_KERNARG_FRAME);
}
#define WF_COLD(st) wf_cold_state()
#define WF_COLD_CAM(cam) wf_cold_camera()
#define WF_COLD_FRAME(fr) wf_cold_frame()
#else
typedef const WfState WfCold;
#define WF_COLD(st) (st)
#define WF_COLD_CAM(cam) (cam)
#define WF_COLD_FRAME(fr) (fr)
#endif

namespace {

__device__ __forceinline__ uint32_t lanemask_lt() { return (uint32_t)__lane_id(); }

// wave-aggregated append of `want` lanes to the list counted by *ctr: returns
// each wanting lane's index
__device__ __forceinline__ uint32_t wave_append(uint32_t *ctr, bool want)
{
    const unsigned long long mask = __ballot(want);
    if (mask == 0) return 0;
    const int lane = __lane_id();
    const int leader = __ffsll((long long)mask) - 1;
    uint32_t base = 0;
    if (lane == leader) base = atomicAdd(ctr, (uint32_t)__popcll(mask));
    base = __shfl(base, leader);
    return base + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
}

// append `want` lanes' rays to ray queue q; returns the entry
__device__ __forceinline__ uint32_t enqueue_ray(const WfState &st, int q, bool want, Vec3D o, Vec3D d)
{
    const uint32_t e = wave_append(st.counts + q, want);
    if (want) {
        st.q_ray[q][2 * (size_t)e] = RtF4{o.x, o.y, o.z, 0.0f};
        st.q_ray[q][2 * (size_t)e + 1] = RtF4{d.x, d.y, d.z, 0.0f};
    }
    return e;
}

// append `want` lanes' paths to path list q
__device__ __forceinline__ void enqueue_path(const WfState &st, int q, bool want, uint32_t slot)
{
    const uint32_t i = wave_append(st.counts + 6 + q, want);
    if (want) st.q_slot[q][i] = slot;
}

// publish ring entry e of the long-path hand-off: the ray, then (after this
// wave's stores are drained and released: the XCD's L2 written back,
// MI355X_MICROARCH.md hand-off rules) the tag wf_long's claims check
template <typename ST>
__device__ __forceinline__ void long_publish(const ST &st, bool to_long, uint32_t e, uint32_t slot, Vec3D o, Vec3D d)
{
    const uint32_t k = e % st.long_cap;
    if (to_long) {
        st.long_ray[2 * (size_t)k] = RtF4{o.x, o.y, o.z, 0.0f};
        st.long_ray[2 * (size_t)k + 1] = RtF4{d.x, d.y, d.z, 0.0f};
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (to_long) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __hip_atomic_store(st.long_ent + k, ((unsigned long long)(e + 1u) << 32) | slot, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
    }
}

// hand `to_long` lanes' paths (state already stored) to wf_long (queue
// kernels: a pixel is handed over at most once per call, and the ring is
// reset per call, so its long_cap = pixels entries never wrap)
__device__ __forceinline__ void publish_long(const WfState &st, bool to_long, uint32_t slot, Vec3D o, Vec3D d)
{
    uint32_t e = 0;
    if (to_long) e = __hip_atomic_fetch_add(st.long_ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    long_publish(st, to_long, e, slot, o, d);
}

// the finisher's hand-off: as publish_long, but the wave reserves its entries
// with one compare-and-swap that never laps an unclaimed entry (a pixel can be
// handed over several times per call when wf_long returns it after each deep
// sample, and chained calls keep the ring running).  Returns false
// (wave-uniform) when the entries would not fit or the ring is closed: the
// lanes then keep their paths.  The path state is stored by the caller first; the pixel is OUT
// (pxo) from here until a finisher takes it back or wf_long finishes it.
template <typename ST>
__device__ __forceinline__ bool publish_long_capped(const ST &st, bool to_long, uint32_t slot, Vec3D o, Vec3D d)
{
    const unsigned long long m = __ballot(to_long);
    const int lane = __lane_id();
    const int leader = __ffsll((long long)m) - 1;
    const uint32_t k = (uint32_t)__popcll(m);
    uint32_t base = 0xffffffffu;
    if (lane == leader) {
        uint32_t r = __hip_atomic_load(st.long_ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        while (true) {
            const uint32_t c = __hip_atomic_load(st.long_ctr + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            // closed (wf_long left: see WF_LONG_CLOSED), the count's 31 bits used up, or a lap of an
            // unclaimed entry (c may be stale-low: conservative): the lanes keep their paths
            if ((r & WF_LONG_CLOSED) || r + k >= WF_LONG_CLOSED || r + k - c > st.long_cap) break;
            if (__hip_atomic_compare_exchange_strong(st.long_ctr, &r, r + k, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                     __HIP_MEMORY_SCOPE_AGENT)) {
                base = r;
                break;
            }
        }
        if (base != 0xffffffffu && st.long_return) // out before the entries can be seen
            __hip_atomic_fetch_add(st.ret_ctr + 3, k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    base = (uint32_t)__shfl((int)base, leader);
    if (base == 0xffffffffu) return false;
    const uint32_t e = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    // (BUSY -> OUT, owed passes kept: one atomic)
    if (to_long && st.long_return)
        __hip_atomic_fetch_xor(st.pxo + slot, RT_PX_OUT ^ RT_PX_BUSY, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    long_publish(st, to_long, e, slot, o, d);
    return true;
}

} // namespace
