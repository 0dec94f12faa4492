// wf_finish_kernels.h — the finishers: wf_finish_bvh (the default whole-call kernel), the guard's wf_check,
// wf_heavy_list, wf_verify and the cooperative wf_finish_coop.
// A part of wavefront.hip's translation unit (included there, once, in the order wf_state.h,
// wf_queue_kernels.h, wf_shade.h, wf_finish_kernels.h, wf_long.h): not for use elsewhere.
#pragma once

namespace {

// a 4-byte load past the CU's L1 (global_load sc1: L2-served), for data another CU released
__device__ __forceinline__ uint32_t ld_sc1(const uint32_t *p)
{
    return __hip_atomic_load(const_cast<uint32_t *>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// a 4-byte write-through store (global_store sc1), for data another CU will read
__device__ __forceinline__ void st_sc1(uint32_t *p, uint32_t v)
{
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// fresh entry e of the whole-call finisher's pixel list -> its pixel: 256
// entries per 16x16-pixel tile, 64 per 8x8-pixel wave tile (wf_start's
// layout); false for a pixel outside the frame or in a row another shard owns
__device__ __forceinline__ bool fresh_pixel(const RtDevFrame &fr, uint32_t e, int &slot)
{
    const uint32_t tiles_x = (uint32_t)(fr.width + 15) / 16u;
    const uint32_t t = e >> 8, w = (e >> 6) & 3u, l = e & 63u;
    const int x = (int)((t % tiles_x) * 16u + (w & 1u) * 8u + (l & 7u));
    const int y = (int)((t / tiles_x) * 16u + (w >> 1) * 8u + (l >> 3));
    if (x >= fr.width || y >= fr.height || !rt_row_owned(fr, y)) return false;
    slot = y * fr.width + x;
    return true;
}

// a sample's path state at its camera ray (trace_path's start, rt/path_tracing.cuh:270-277)
template <typename P>
__device__ __forceinline__ void begin_path(P &p)
{
    p.T = rt_v3(1.0f, 1.0f, 1.0f);
    p.L = rt_v3(0.0f, 0.0f, 0.0f);
    p.inside = false;
    p.prev_type = PRIMARY;
    p.depth = 1;
    p.shadow = false;
    p.dual = false;
    p.ext_live = false;
}

} // namespace

// Finisher with the BVH-bounded traversal (bvh_trace.h): every lane runs one
// path to the end of its pixel's passes (trace + shade in registers,
// megakernel style) and then takes the next queued path (wave-aggregated
// atomic on counts[4]); a path deeper than long_depth goes on in wf_long.
// With the bounded traversal this runs the WHOLE call (wf_start's path list:
// no queue iterations), see rt_launch_wavefront.  COUNT: the traversal's own
// work (trace_bvh) and the reference's shading counters.
// WAVES: the occupancy it is built for — WF_FIN_BVH_WAVES (96 VGPRs, the rest
// spilled) when the chip is full of its waves; 1 (no register cap, no spills)
// for a frame whose pixels fill at most WF_FIN_SMALL_WAVES waves per SIMD, where
// the occupancy is the pixel count's anyway and every spill's latency shows
template <bool COUNT, int WAVES = WF_FIN_BVH_WAVES>
__global__ void __launch_bounds__(WF_BLOCK, WAVES) wf_finish_bvh(RtDevScene sc, RtDevFrame fr, RtDevCamera cam,
                                                                 WfState st, int q)
{
    __shared__ uint32_t s_node[WF_BVH_LDS * WF_BLOCK];
    __shared__ float s_entry[WF_BVH_LDS * WF_BLOCK];
    const int tid = threadIdx.x;
    const int wbase = __builtin_amdgcn_readfirstlane(tid & ~63); // (wave-uniform)
    LaneStack<WF_BVH_LDS> stk{s_node + wbase, s_entry + wbase, WF_BLOCK, st.spill + (blockIdx.x * WF_BLOCK + wbase),
                              st.spill_threads};
    Cnt c;
    if (COUNT) c.zero();
    // fresh: this call's pixels, 256 entries per 16x16-pixel tile (fresh_pixel); else the paths of path list q
    // (fresh: the listed heavy pixels first, then the tiles)
    const uint32_t n_heavy = st.fresh && st.heavy_list ? *st.heavy_n : 0u;
    const uint32_t n = st.fresh ? n_heavy + st.fresh_n : st.counts[6 + q];
    const int limit = fr.max_depth > 0 ? fr.max_depth : RT_WATCHDOG_BOUNCES;
    const int lane = __lane_id();
    // (RT_COLD_ARGS, wf_state.h: the loop reads st.fresh, long_return, linger, long_depth, chk, chk_mask and the stack's
    // spill base from registers; every other field of the state where it is used, through WF_COLD)
    if (lane == 0) {
        unsigned long long *const ret_word = reinterpret_cast<unsigned long long *>(st.ret_ctr);
        // the call's finisher has started: from here wf_long waits for its producers (WF_FIN_STARTED)
        if (st.fin_live && !(__hip_atomic_load(st.fin_live, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & WF_FIN_STARTED))
            __hip_atomic_fetch_or(st.fin_live, WF_FIN_STARTED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (st.long_return) // this wave is alive: wf_long may return pixels to it
            __hip_atomic_fetch_add(ret_word, 1ull << 32, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (st.span) atomicMin(st.span, __builtin_amdgcn_s_memrealtime());
        if (st.long_log && blockIdx.x == 0 && threadIdx.x == 0) st.long_log[0] = __builtin_amdgcn_s_memrealtime();
    }
#if WF_NEE_LDS
    __shared__ float s_nee[10 * WF_BLOCK];
    PathRegsL p;
    p.rp.w = s_nee + wbase;
    p.cont.w = s_nee + 3 * WF_BLOCK + wbase;
    p.snorm.w = s_nee + 6 * WF_BLOCK + wbase;
    p.light.w = reinterpret_cast<int *>(s_nee + 9 * WF_BLOCK) + wbase;
#else
    PathRegs p;
#endif
    p.slot = 0;
    p.ro = p.rd = rt_v3(0, 0, 0);
    bool active = false, exhausted = false; // exhausted: this lane found the path list empty
    bool rel = false;                       // (fresh) the lane's pixel has no passes left: let it go
    unsigned long long idle_since = 0;      // (lane 0) when the wave first had nothing to do
    uint32_t quiet_trips = 0;               // (lane 0) idle loop trips in a row with no wf_long path running
    uint32_t idle_trips = 0;                // (lane 0) idle loop trips in a row
    bool seated = false;                    // (lane 0) holds a linger seat
    // a wave whose s_min queries ran WF_BVH_BUDGET bodies parks the unfinished ones (a lane's state in LDS, the
    // stack in place) and resumes them in its next loop trip: the rest of the wave shades meanwhile
    __shared__ uint32_t s_pk_cur[WF_BLOCK];
    __shared__ int s_pk_sp[WF_BLOCK];
    __shared__ float s_pk_best[WF_BLOCK];
    __shared__ int s_pk_tk[WF_BLOCK];
    // RT_PARK_KD: the lane's ray is past its query and not covered by the T* certificate — only the KD
    // descent is left (s_min and its slot in s_pk_best / s_pk_tk).  One such lane must not make its wave
    // walk a descent alone: the pending descents run together, in a trip where WF_KD_PEND_MIN lanes wait
    // for theirs or no lane of the wave has anything else to do.
    int parked = RT_PARK_DONE;
    while (true) {
        // (fresh) pixels whose passes are done are let go — unless a later chained call queued
        // passes for them meanwhile: those run next, in the pixel's order (its state is this lane's).
        // (The next claimer is a later launch — chained finishers run one after the other — whose
        // kernel boundary orders this lane's stores before its loads.)
        while (st.fresh && __any(rel)) {
            if (rel) {
                WfCold &cs = WF_COLD(st);
                uint32_t x = RT_PX_BUSY;
                if (__hip_atomic_compare_exchange_strong(cs.pxo + p.slot, &x, 0u, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                         __HIP_MEMORY_SCOPE_AGENT)) {
                    rel = false;
                } else {
                    x = __hip_atomic_exchange(cs.pxo + p.slot, RT_PX_BUSY, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    const uint32_t owed = x & RT_PX_PASSES;
                    __hip_atomic_fetch_max(cs.ret_ctr + 5, owed, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_fetch_add(cs.ret_ctr + 6, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    const RtDevFrame cf = WF_COLD_FRAME(fr);
                    atomicAdd(cf.dev_stats + RT_DEV_OWED_PIXELS, 1ull);
                    atomicAdd(cf.dev_stats + RT_DEV_OWED_PASSES, (unsigned long long)owed);
                    p.passes_left = (int)owed;
                    const Vec3D fb = cf.fb[p.slot];
                    const float sq = cf.sq[p.slot];
                    const int count = cf.count[p.slot];
                    if (start_sample<COUNT>(cf, WF_COLD_CAM(cam), (int)p.slot, p.passes_left, p.rng, fb, sq, count, p.ro, p.rd,
                                            c)) {
                        begin_path(p);
                        rel = false;
                        active = true;
                    }
                }
            }
        }
        if (st.long_return) {
            // free lanes take pixels wf_long returned BEFORE fresh ones (one
            // compare-and-swap per wave): a returned pixel is mid-chain — it may
            // carry the passes of chained calls that skipped it (pxo) — and
            // started only at the end of the path list it would end the call late.
            // Chained calls (no linger): only while the path list lasts — the call's
            // tail leaves later returns to the next call's (or the drain's) finisher
            const bool chained = st.linger == 0ull;
            const bool idle = !active && !(chained && exhausted);
            const unsigned long long im = __ballot(idle);
            if (im) {
                WfCold &cs = WF_COLD(st);
                unsigned long long *const ret_word = reinterpret_cast<unsigned long long *>(cs.ret_ctr);
                uint32_t *const ret_claimed = cs.ret_ctr + 2;
                const int leader = __ffsll((long long)im) - 1;
                uint32_t base = 0, got = 0;
                if (lane == leader) {
                    uint32_t c0 = __hip_atomic_load(ret_claimed, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    const uint32_t r =
                        (uint32_t)__hip_atomic_load(ret_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    const uint32_t want_n = (uint32_t)__popcll(im);
                    uint32_t take = r > c0 ? (r - c0 < want_n ? r - c0 : want_n) : 0u;
                    if (take && chained &&
                        __hip_atomic_load(cs.counts + 4, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= n)
                        take = 0u;
                    if (take && __hip_atomic_compare_exchange_strong(ret_claimed, &c0, c0 + take, __ATOMIC_RELAXED,
                                                                     __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
                        base = c0;
                        got = take;
                    }
                }
                base = (uint32_t)__shfl((int)base, leader);
                got = (uint32_t)__shfl((int)got, leader);
                const uint32_t rank = (uint32_t)__popcll(im & ((1ull << lane) - 1ull));
                if (idle && rank < got) {
                    // reserved by a running wf_long wave, which publishes it right after (store
                    // in flight): a bounded wait — expired, the pixel stays out (wf_verify
                    // reports it stranded) rather than the wave spinning on
                    const uint32_t e = base + rank;
                    unsigned long long v = 0;
                    bool pub = false;
                    for (uint32_t spin = 0; spin < WF_SPIN_TRIPS; ++spin) {
                        v = __hip_atomic_load(cs.ret_ring + e % cs.long_cap, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        pub = (uint32_t)(v >> 32) == e + 1u;
                        if (pub) break;
                        __builtin_amdgcn_s_sleep(1);
                    }
                    if (!pub) {
                        atomicAdd(WF_COLD_FRAME(fr).dev_stats + RT_DEV_LONG_QUIT, 1ull);
                    } else {
                        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                        __hip_atomic_fetch_sub(cs.ret_ctr + 3, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        active = true;
                        const RtDevFrame cf = WF_COLD_FRAME(fr);
                        first_ray(cs, cf, (uint32_t)v, p);
                        // back from wf_long: no longer OUT but BUSY (this lane's); plus the passes chained
                        // calls queued meanwhile
                        const uint32_t owed = __hip_atomic_exchange(cs.pxo + (uint32_t)v, RT_PX_BUSY, __ATOMIC_RELAXED,
                                                                    __HIP_MEMORY_SCOPE_AGENT);
                        p.passes_left += (int)(owed & RT_PX_PASSES);
                        if (owed & RT_PX_PASSES) { // (RT_DEBUG_CALL_LOG: most passes owed, pixels owed; RtDeviations)
                            __hip_atomic_fetch_max(cs.ret_ctr + 5, owed & RT_PX_PASSES, __ATOMIC_RELAXED,
                                                   __HIP_MEMORY_SCOPE_AGENT);
                            __hip_atomic_fetch_add(cs.ret_ctr + 6, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                            atomicAdd(cf.dev_stats + RT_DEV_OWED_PIXELS, 1ull);
                            atomicAdd(cf.dev_stats + RT_DEV_OWED_PASSES, (unsigned long long)(owed & RT_PX_PASSES));
                        }
                    }
                }
            }
        }
        if (st.fresh) {
            // this call's pixels (wf_start's work, in its 8x8-pixel wave tiles): a lane claims its
            // pixel (BUSY) unless another holder still has it — a previous chained call's finisher
            // lane or wf_long —, which then owes it this call's passes and runs them next
            // (a lane that found the list run out stays out: idle trips must not keep adding to
            // the cursor — a lingering wave's trips wrapped it past 2^32 and re-ran the call's
            // pixels)
            bool claim = !active && !rel && !exhausted, started = false, acq = false;
            while (__any(claim)) {
                WfCold &cs = WF_COLD(st);
                const RtDevFrame cf = WF_COLD_FRAME(fr);
                const unsigned long long m = __ballot(claim);
                const int leader = __ffsll((long long)m) - 1;
                uint32_t base = 0;
                if (lane == leader) base = atomicAdd(cs.counts + 4, (uint32_t)__popcll(m));
                base = __shfl(base, leader);
                if (claim) {
                    const uint32_t e = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
                    int slot = 0;
                    if (e >= n) {
                        claim = false;
                        exhausted = true;
                    } else if (e < n_heavy ? (slot = (int)cs.heavy_list[e], true)
                                           : fresh_pixel(cf, e - n_heavy, slot) &&
                                                 !(cs.heavy_list && cs.listed[slot] == cs.call_id)) {
                        uint32_t x = __hip_atomic_load(cs.pxo + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        while (true) {
                            if (x & (RT_PX_OUT | RT_PX_BUSY)) { // held: owed this call's passes
                                if (__hip_atomic_compare_exchange_strong(cs.pxo + slot, &x, x + (uint32_t)cf.passes,
                                                                         __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                                         __HIP_MEMORY_SCOPE_AGENT))
                                    break;
                            } else if (__hip_atomic_compare_exchange_strong(cs.pxo + slot, &x, RT_PX_BUSY,
                                                                            __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                                            __HIP_MEMORY_SCOPE_AGENT)) {
                                claim = false;
                                started = true;
                                acq = (x & RT_PX_REL) != 0u; // (released by wf_long, which runs beside this)
                                p.slot = (uint32_t)slot;
                                break;
                            }
                        }
                    }
                }
            }
            // (a pixel whose last holder was wf_long, running beside this finisher, was released with
            // plain stores + an agent release before the word said free (LONGDONE): read it after an
            // agent acquire.  sc1 loads alone are no acquire for plain-stored bytes
            // (MI355X_MICROARCH.md, Valid forms): this XCD's L2 may hold the line from a neighbouring
            // pixel read earlier.  A pixel last held by an earlier launch needs none: the launch
            // boundary is the release / acquire.)
            if (__any(acq)) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            if (started) { // the pixel's state and its first pass (wf_start's)
                const RtDevFrame cf = WF_COLD_FRAME(fr);
                const uint32_t slot = p.slot;
                p.rng = ld_sc1(cf.rng + slot);
                Vec3D fb = rt_v3(0.0f, 0.0f, 0.0f);
                float sq = 0.0f;
                int count = 0;
                if (cf.reset) { // reset_frame (rt/render.cuh:18-34)
                    cf.fb[slot] = fb;
                    cf.sq[slot] = sq;
                    cf.count[slot] = count;
                } else {
                    const uint32_t *f3 = reinterpret_cast<const uint32_t *>(cf.fb + slot);
                    fb = rt_v3(__uint_as_float(ld_sc1(f3)), __uint_as_float(ld_sc1(f3 + 1)), __uint_as_float(ld_sc1(f3 + 2)));
                    sq = __uint_as_float(ld_sc1(reinterpret_cast<const uint32_t *>(cf.sq + slot)));
                    count = (int)ld_sc1(reinterpret_cast<const uint32_t *>(cf.count + slot));
                }
                p.passes_left = cf.passes;
                if (start_sample<COUNT>(cf, WF_COLD_CAM(cam), (int)slot, p.passes_left, p.rng, fb, sq, count, p.ro, p.rd, c)) {
                    begin_path(p);
                    active = true;
                } else {
                    rel = true; // no sample this call (adaptive test): let it go
                }
            }
        } else {
            const bool need = !active && !exhausted;
            const unsigned long long m = __ballot(need);
            if (m) {
                WfCold &cs = WF_COLD(st);
                const int leader = __ffsll((long long)m) - 1;
                uint32_t base = 0;
                if (lane == leader) base = atomicAdd(cs.counts + 4, (uint32_t)__popcll(m));
                base = __shfl(base, leader);
                if (need) {
                    const uint32_t e = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
                    if (e >= n) {
                        exhausted = true;
                    } else {
                        active = true;
                        first_ray(cs, WF_COLD_FRAME(fr), cs.q_slot[q][e], p);
                    }
                }
            }
        }
        if (!__any(active || rel)) {
            if (!st.long_return) break; // every lane exhausted
            WfCold &cs = WF_COLD(st);
            unsigned long long *const ret_word = reinterpret_cast<unsigned long long *>(cs.ret_ctr);
            uint32_t *const ret_claimed = cs.ret_ctr + 2;
            if (st.linger == 0ull) { // chained: returns left are the next call's (or the drain's)
                if (lane == 0) __hip_atomic_fetch_sub(ret_word, 1ull << 32, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                break;
            }
            // leave only while every reserved return is claimed (else: claim them next round), and
            // while pixels are out in wf_long linger for them — bounded: st.linger ticks, and
            // WF_FIN_QUIET_TRIPS trips with no wf_long path running (where wf_long cannot run
            // beside the finisher — counter collection serialises the two launches — lingering
            // would only hold the finisher's end, and the next launch, up), WF_FIN_LINGER_TRIPS in all
            int leave = 0;
            if (lane == 0) {
                if (idle_since == 0) idle_since = __builtin_amdgcn_s_memrealtime();
                if (__hip_atomic_load(cs.long_ctr + 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u)
                    ++quiet_trips;
                else
                    quiet_trips = 0;
                ++idle_trips;
                bool out = quiet_trips < WF_FIN_QUIET_TRIPS && idle_trips < WF_FIN_LINGER_TRIPS &&
                           __hip_atomic_load(cs.ret_ctr + 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u;
                // only WF_FIN_LINGER_WAVES waves linger (a seat each, kept until they leave): the
                // others leave their slots to wf_long, which the deep paths are waiting for
                if (out && !seated) {
                    if (__hip_atomic_fetch_add(cs.ret_ctr + 4, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) <
                        WF_FIN_LINGER_WAVES)
                        seated = true;
                    else
                        out = false;
                }
                unsigned long long w = __hip_atomic_load(ret_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const uint32_t cl = __hip_atomic_load(ret_claimed, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if ((uint32_t)w == cl &&
                    (!out || __builtin_amdgcn_s_memrealtime() - idle_since > st.linger) &&
                    __hip_atomic_compare_exchange_strong(ret_word, &w, w - (1ull << 32), __ATOMIC_RELAXED,
                                                         __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
                    leave = 1;
                    // (pixels still out: wf_long, finding no finisher alive, finishes them itself)
                    if (out) atomicAdd(WF_COLD_FRAME(fr).dev_stats + RT_DEV_LINGER_EXP, 1ull);
                }
            }
            if (__shfl(leave, 0)) break;
            __builtin_amdgcn_s_sleep(8);
            continue;
        }
        idle_since = 0;
        quiet_trips = 0;
        idle_trips = 0;
        bool to_long = false;
#if RT_KD_CERT
        const unsigned long long kd_pend = __ballot(active && parked == RT_PARK_KD);
        const bool run_kd = kd_pend != 0ull && (__popcll(kd_pend) >= WF_KD_PEND_MIN ||
                                                __ballot(active && parked != RT_PARK_KD) == 0ull);
        if (active && (parked != RT_PARK_KD || run_kd)) {
#else
        if (active) {
#endif
            float bx = 0.0f, by = 0.0f, bz = 0.0f;
            int hit;
            BvhPark pk{0u, 0, 0.0f, -1};
            if (parked != RT_PARK_DONE) pk = BvhPark{s_pk_cur[tid], s_pk_sp[tid], s_pk_best[tid], s_pk_tk[tid]};
            // (the budget is a compile-time constant in the product instantiation: no scalar joins its hot set.
            // Tests run the counting instantiation at budget 1, RT_DEBUG_BUDGET1.)
            const int budget = COUNT && (WF_COLD(st).chk_fault & WF_DEBUG_BUDGET1) ? 1 : WF_BVH_BUDGET;
            parked = trace_bvh_park<COUNT>(sc, p.ro, p.rd, hit, bx, by, bz, stk, c, budget, parked, true, pk);
            const bool done = parked == RT_PARK_DONE;
            if (!done) {
                s_pk_cur[tid] = pk.cur;
                s_pk_sp[tid] = pk.sp;
                s_pk_best[tid] = pk.best;
                s_pk_tk[tid] = pk.tk;
            }
            // run-time exactness guard: a deterministic sample of the rays, with the
            // bounded result, is queued for wf_check's plain KD re-trace
            if (!COUNT && st.chk && done) {
                uint32_t h = p.slot * 0x9E3779B1u ^ (uint32_t)p.passes_left * 0x85EBCA77u ^
                             (uint32_t)p.depth * 0xC2B2AE3Du ^ (p.shadow ? 0x27D4EB2Fu : 0u);
                h ^= h >> 15;
                h *= 0x2C1B3C6Du;
                h ^= h >> 12;
                const bool rec = (h & st.chk_mask) == 0u;
                if (__any(rec)) {
                    WfCold &cs = WF_COLD(st);
                    const uint32_t i = wave_append(cs.chk_ctr, rec);
                    if (rec && i < cs.chk_cap) {
                        cs.chk[3 * (size_t)i] =
                            RtF4{p.ro.x, p.ro.y, p.ro.z, __int_as_float((cs.chk_fault & 1) ? (hit >= 0 ? hit ^ 1 : 0) : hit)};
                        cs.chk[3 * (size_t)i + 1] = RtF4{p.rd.x, p.rd.y, p.rd.z, bx};
                        cs.chk[3 * (size_t)i + 2] = RtF4{by, bz, 0.0f, 0.0f};
                    }
                }
            }
            if (done) {
                const RtDevFrame cf = WF_COLD_FRAME(fr);
                const bool want = shade_step<COUNT>(sc, cf, WF_COLD_CAM(cam), p, hit, bx, by, bz, limit, c);
                // a path deeper than long_depth goes on in wf_long (64 lanes per ray)
                to_long = want && st.long_depth > 0 && p.depth > st.long_depth;
                if (!want || to_long) store_regs(WF_COLD(st), cf, p);
                if (!want) {
                    active = false;
                    rel = st.fresh != 0; // (the pixel's passes are done: let go at the top of the loop)
                }
            }
        }
        if (__any(to_long)) {
            WfCold &cs = WF_COLD(st);
            if (publish_long_capped(cs, to_long, p.slot, p.ro, p.rd) && to_long) {
                active = false;
                if (cs.heavy) { // (first in the next call's list: the more hand-offs, the earlier)
                    const uint8_t h = cs.heavy[p.slot];
                    if (h < 255) cs.heavy[p.slot] = (uint8_t)(h + 1);
                }
            }
        }
    }
    if (COUNT) {
        flush_counters(c, fr.counters);
        flush_cert_counters(c, fr.dev_stats);
    }
    WfCold &ce = WF_COLD(st);
    if (ce.span && lane == 0) atomicMax(ce.span + 1, __builtin_amdgcn_s_memrealtime());
    if (ce.fin_live) { // this wave's hand-offs are published: the persistent wf_long may stop once all are past here
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        if (lane == 0) __hip_atomic_fetch_sub(ce.fin_live, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// The run-time exactness guard's second half: every ray wf_finish_bvh
// recorded is traced again with the plain KD traversal (trace(), i.e.
// trace_ray, rt/trace_ray.cuh:244-318) and compared bit for bit with the
// bounded result (triangle, barycentrics).  Counts checks and mismatches in
// the deviation statistics and keeps the first mismatching ray.  One ray per
// lane, grid-stride within the spill area (grid blocks).
__global__ void __launch_bounds__(WF_BLOCK) wf_check(RtDevScene sc, WfState st, unsigned long long *dev)
{
    __shared__ uint32_t s_node[WF_LDS_STACK * WF_BLOCK];
    __shared__ float s_entry[WF_LDS_STACK * WF_BLOCK];
    const int tid = threadIdx.x;
    const int gtid = blockIdx.x * WF_BLOCK + tid;
    Stack<WF_LDS_STACK> stk{s_node + tid, s_entry + tid, WF_BLOCK, st.spill + gtid, st.spill_threads};
    Cnt c;
    uint32_t n = *st.chk_ctr;
    if (n > st.chk_cap && gtid == 0) atomicAdd(dev + RT_DEV_CHK_DROP, (unsigned long long)(n - st.chk_cap));
    n = n < st.chk_cap ? n : st.chk_cap;
    unsigned long long checked = 0, bad = 0;
    // records over the waves first (record e on wave e % waves, lane e / waves): a small call's
    // few records run one or two per wave, each re-trace's node fetches alone in its wave, not
    // 64 in lockstep in the first waves (the slowest re-trace bounds the kernel, and the chained
    // call two later waits for it: its records reuse this parity)
    const uint32_t waves = gridDim.x * (WF_BLOCK / 64);
    const uint32_t first = (uint32_t)(tid & 63) * waves + blockIdx.x * (WF_BLOCK / 64) + (uint32_t)(tid >> 6);
    for (uint32_t e = first; e < n; e += gridDim.x * WF_BLOCK) {
        const RtF4 a = st.chk[3 * (size_t)e], b = st.chk[3 * (size_t)e + 1], q = st.chk[3 * (size_t)e + 2];
        const Vec3D o = rt_v3(a.x, a.y, a.z), d = rt_v3(b.x, b.y, b.z);
        float bx = 0.0f, by = 0.0f, bz = 0.0f;
        const int hit = trace<false>(sc, o, d, bx, by, bz, stk, c);
        ++checked;
        const bool same = hit == __float_as_int(a.w) &&
                          (hit < 0 || (__float_as_uint(bx) == __float_as_uint(b.w) &&
                                       __float_as_uint(by) == __float_as_uint(q.x) &&
                                       __float_as_uint(bz) == __float_as_uint(q.y)));
        if (!same) {
            ++bad;
            if (atomicCAS(dev + RT_DEV_MISRAY, 0ull, 1ull) == 0ull) { // the first mismatch: its ray
                dev[RT_DEV_MISRAY + 1] = (unsigned long long)__float_as_uint(o.x) << 32 | __float_as_uint(o.y);
                dev[RT_DEV_MISRAY + 2] = (unsigned long long)__float_as_uint(o.z) << 32 | __float_as_uint(d.x);
                dev[RT_DEV_MISRAY + 3] = (unsigned long long)__float_as_uint(d.y) << 32 | __float_as_uint(d.z);
            }
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        checked += __shfl_xor(checked, off);
        bad += __shfl_xor(bad, off);
    }
    if ((tid & 63) == 0) {
        if (checked) atomicAdd(dev + RT_DEV_CHECKED, checked);
        if (bad) atomicAdd(dev + RT_DEV_MISMATCH, bad);
    }
}

// The join's check of the hand-off protocol (after every finisher, wf_long and
// drain of the workspace is done): a pixel still OUT was handed to wf_long and
// never came back, one still BUSY was never let go by a finisher lane — its
// frame misses passes.  Counts such pixels (and releases
// them, so later calls run them again) and the protocol's counters that must
// be balanced by now: pixels out, returns reserved but unclaimed, hand-off
// entries reserved but unclaimed, finisher waves still registered alive.
// res: [0] stranded pixels, [1..4] those counters (accumulated until the host reads them).
// Heavy pixels first: the pixels marked heavy (a path of theirs went to wf_long
// in an earlier call) that this call renders, listed (wave-aggregated atomic:
// any order — a pixel's passes run in its own order whoever takes it first)
// and tagged with the call so the finisher's tile entries skip them.  The
// deep-path-prone pixels then start their chains at the call's start instead
// of wherever their tile falls: their deep samples end inside the call rather
// than in the chain's drain.
__global__ void __launch_bounds__(WF_BLOCK) wf_heavy_list(RtDevFrame fr, WfState st, uint32_t call_id,
                                                           uint32_t lo, uint32_t hi)
{
    const uint32_t n = (uint32_t)fr.width * (uint32_t)fr.height;
    const int lane = __lane_id();
    // (wave-uniform loop: every lane of the wave reaches the ballot)
    for (uint32_t w0 = blockIdx.x * WF_BLOCK + (threadIdx.x & ~63u); w0 < n; w0 += WF_BLOCK * gridDim.x) {
        const uint32_t i = w0 + (uint32_t)lane;
        // (pixels handed over lo..hi-1 times so far: the heaviest are listed by the first launch)
        const uint32_t h = i < n ? (uint32_t)st.heavy[i] : 0u;
        const bool take = h >= lo && h < hi && rt_row_owned(fr, (int)(i / (uint32_t)fr.width));
        const unsigned long long m = __ballot(take);
        if (!m) continue;
        const int leader = __ffsll((long long)m) - 1;
        uint32_t base = 0;
        if (lane == leader) base = atomicAdd(st.heavy_n, (uint32_t)__popcll(m));
        base = (uint32_t)__shfl((int)base, leader);
        if (take) {
            st.heavy_list[base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = i;
            st.listed[i] = call_id;
        }
    }
}

__global__ void __launch_bounds__(WF_BLOCK) wf_verify(WfState st, uint32_t n, uint32_t *res, unsigned long long *dev)
{
    uint32_t out = 0;
    for (uint32_t i = blockIdx.x * WF_BLOCK + threadIdx.x; i < n; i += gridDim.x * WF_BLOCK) {
        const uint32_t x = st.pxo[i];
        if (x) { // (free-after-a-concurrent-holder words become plain free: the join ordered everything)
            out += (x & (RT_PX_OUT | RT_PX_BUSY)) ? 1u : 0u;
            st.pxo[i] = 0u;
        }
    }
    for (int off = 32; off > 0; off >>= 1) out += __shfl_xor(out, off);
    if ((threadIdx.x & 63) == 0 && out) {
        atomicAdd(res, out);
        atomicAdd(dev + RT_DEV_STRANDED, (unsigned long long)out);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const unsigned long long rw = *reinterpret_cast<const unsigned long long *>(st.ret_ctr);
        res[1] += st.ret_ctr[3];
        res[2] += (uint32_t)rw - st.ret_ctr[2];
        res[3] += (st.long_ctr[0] & ~WF_LONG_CLOSED) - st.long_ctr[1];
        res[4] += (uint32_t)(rw >> 32);
    }
}

// Cooperative finisher: runs queued paths to the end of their passes in
// registers (shade_step right after each ray query), megakernel style, while
// the whole wave tests leaf entries for its live rays together (coop_round).
// Each wave keeps up to `ppw` (1..64) paths in flight, one per lane; a lane
// whose path is done takes the next queue entry (wave-aggregated atomic on
// counts[4]).  With ppw = 1 a lone long glass path gets its leaves tested 64
// entries at a time instead of one.
template <bool COUNT>
__global__ void __launch_bounds__(WF_BLOCK, WF_FIN_OCC) wf_finish_coop(RtDevScene sc, RtDevFrame fr, RtDevCamera cam, WfState st,
                                                           int q, int ppw, int cap, int postpone, int wide)
{
    __shared__ uint32_t s_node[WF_LDS_STACK * WF_BLOCK];
    __shared__ float s_entry[WF_LDS_STACK * WF_BLOCK];
    __shared__ unsigned long long s_key[WF_BLOCK];
    __shared__ CoopCand s_list[(WF_BLOCK / 64) * WF_COOP_LIST];
    __shared__ int s_mark[2 * WF_BLOCK]; // 128 per wave: chunk_owner marks + junk slots
    __shared__ WideItem s_wide[(WF_BLOCK / 64) * WIDE_CAP];
    const int tid = threadIdx.x;
    const int gtid = blockIdx.x * WF_BLOCK + tid;
    const int lane = __lane_id();
    const int wave = tid >> 6;
    Stack<WF_LDS_STACK> stk{s_node + tid, s_entry + tid, WF_BLOCK, st.spill + gtid, st.spill_threads};
    unsigned long long *wkey = s_key + wave * 64;
    CoopCand *list = s_list + wave * WF_COOP_LIST;
    const CoopLds w{wkey, list, s_mark + wave * 128};
    Cnt c;
    if (COUNT) c.zero();
    const uint32_t n = st.counts[6 + q]; // paths of path list q
    uint32_t *fetch = st.counts + 4;
    const int limit = fr.max_depth > 0 ? fr.max_depth : RT_WATCHDOG_BOUNCES;

    PathRegs p;
    p.slot = 0;
    p.ro = p.rd = rt_v3(0, 0, 0);
    CoopRay r;
    coop_idle(r);
    int hit = -1;
    float bx = 0.0f, by = 0.0f, bz = 0.0f;
    bool active = false;              // the lane holds a path
    bool exhausted = lane >= ppw;     // no more queue entries for this lane
    bool pending = false;             // a finished ray query waiting for shade_step
    while (true) {
        // ---- idle lanes take the next queued paths
        if (!active && !exhausted) {
            const uint32_t e = wave_next_index(fetch, lane);
            if (e >= n) {
                exhausted = true;
            } else {
                active = true;
                first_ray(st, fr, st.q_slot[q][e], p);
                if (COUNT) c.v[RT_CNT_RAY]++;
                if (!coop_begin(sc, r, p.ro, p.rd)) {
                    pending = true;
                    hit = -1;
                }
            }
        }
        while (pending) { // shade, and start the path's next ray (a scene-box miss is shaded at once)
            pending = false;
            if (shade_step<COUNT>(sc, fr, cam, p, hit, bx, by, bz, limit, c)) {
                if (COUNT) c.v[RT_CNT_RAY]++;
                if (!coop_begin(sc, r, p.ro, p.rd)) {
                    pending = true;
                    hit = -1;
                }
            } else {
                store_regs(st, fr, p);
                active = false;
            }
        }
        // here every active lane has a live ray
        const unsigned long long lm = __ballot(r.live);
        if (!lm) {
            if (__all(exhausted)) break;
            continue;
        }
        if (__popcll(lm) <= wide) {
            // few rays left in the wave: each is traced by all 64 lanes, one
            // after the other (wide_resume picks up a ray mid-traversal from
            // its lane's stack) — a cooperative round would advance them
            // together, but at ~5 node fetches per round instead of a level
            // of the whole frontier
            const WideLds W{s_wide + wave * WIDE_CAP, WIDE_CAP, wkey, reinterpret_cast<float *>(wkey + 1), w.mark};
            for (unsigned long long mm = lm; mm; mm &= mm - 1) {
                const int owner = __ffsll((long long)mm) - 1;
                const int ot = wave * 64 + owner;
                const Stack<WF_LDS_STACK> so{s_node + ot, s_entry + ot, WF_BLOCK,
                                             st.spill + blockIdx.x * WF_BLOCK + ot, st.spill_threads};
                int t;
                float x, y, z;
                wide_resume<COUNT>(sc, r, owner, so, W, t, x, y, z, c);
                if (lane == owner) {
                    hit = t;
                    bx = x;
                    by = y;
                    bz = z;
                    r.live = false;
                    pending = true;
                }
            }
            continue;
        }
        if (coop_round<COUNT>(sc, r, stk, w, cap, postpone, hit, bx, by, bz, c)) pending = true;
    }
    if (COUNT) {
        flush_counters(c, fr.counters);
        flush_finish_counters(c, fr.counters);
    }
}
