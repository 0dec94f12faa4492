// wf_long.h — the deep paths' kernel.
// A part of wavefront.hip's translation unit (included there, once, in the order wf_state.h,
// wf_queue_kernels.h, wf_shade.h, wf_finish_kernels.h, wf_long.h): not for use elsewhere.
#pragma once

// Long paths (total internal reflection in glass runs to 10^4 bounces and
// more) would otherwise hold up the end of the call one bounce per queue
// iteration or one lane at a time.  Paths deeper than st.long_depth are handed
// to this kernel through the hand-off ring; each wave claims the next
// PUBLISHED entry in order (compare-and-swap on the claim counter, never an
// entry whose publication is still in flight) and runs that path with every
// ray traced by all 64 lanes (wide_trace; bounded whole calls: wide_bvh.h), lane 0 shading.
//
// Two launch forms:
//  * whole-call mode (st.fin_live != nullptr): ONE persistent launch per call
//    on its own stream, beside the finisher; a wave leaves once every finisher
//    wave of its call is past its last hand-off (fin_live == 0) and every
//    reserved entry is claimed.  It runs a path only to the end of its deep
//    SAMPLE, then returns the pixel to a live finisher (return ring) or, with
//    none alive, runs the pixel's remaining passes itself — including passes
//    that later chained calls owe it (pxo) — and releases it (LONGDONE).
//  * queue mode (fin_live == nullptr): slices on the caller's stream, kicked
//    by the pipelines' host threads; a wave with nothing to claim waits only
//    while another path is running, the final slice drains the rest; a path
//    runs to the end of its pixel's passes.
// Neither form waits for a kernel that is not resident (see the cross-kernel
// waits at WF_FIN_STARTED): a persistent wave waits for its finisher only once
// a finisher wave has started, and closes the ring and leaves when none has
// within WF_LONG_START_TRIPS — so neither can deadlock when the runtime maps
// these streams onto one hardware queue or a profiler serialises dispatches.
template <bool COUNT>
__global__ void __launch_bounds__(WF_BLOCK, WF_LONG_WAVES) wf_long(RtDevScene sc, RtDevFrame fr, RtDevCamera cam, WfState st,
                                                    int final_slice)
{
    __shared__ __attribute__((aligned(16))) WideItem s_wide[(WF_BLOCK / 64) * WIDE_CAP]; // (also wide_smin's 8-B items)
    static_assert(WSM_LDS_BYTES <= WIDE_CAP * sizeof(WideItem), "the wide s_min query's lists reuse the wave's frontier");
    static_assert(WSM_KD_STACK * 8 <= 128 * sizeof(int), "the bounded KD phase's stack reuses the wave's chunk_owner marks");
    __shared__ unsigned long long s_key[(WF_BLOCK / 64) * 4];
    __shared__ __attribute__((aligned(8))) int s_mark[2 * WF_BLOCK]; // 128 per wave: chunk_owner marks + junk slots
    if (WF_LONG_PRIO > 0) __builtin_amdgcn_s_setprio(WF_LONG_PRIO);
    const int lane = __lane_id();
    const int wave = threadIdx.x >> 6;
    const WideLds W{s_wide + wave * WIDE_CAP, WIDE_CAP, s_key + wave * 4,
                    reinterpret_cast<float *>(s_key + wave * 4 + 1), s_mark + wave * 128};
    Cnt c;
    if (COUNT) c.zero();
    const int limit = fr.max_depth > 0 ? fr.max_depth : RT_WATCHDOG_BOUNCES;
    // (RT_COLD_ARGS, wf_state.h: a bounce reads st.long_wide and st.long_return from registers; the claim, the
    // return and the release read their fields of the state where they use them, through WF_COLD)
    const bool persist = st.fin_live != nullptr;
    unsigned long long t_idle = __builtin_amdgcn_s_memrealtime(); // (chain window: since entries last flowed)
    unsigned long long t_net = t_idle; // safety net: since anything that could still bring work last held
    unsigned long long t_pub = 0;      // since entry e_pub was first seen reserved but unpublished
    // (the same bounds in loop trips: s_memrealtime stands still under counter collection)
    uint32_t n_idle = 0, n_net = 0, n_pub = 0, n_start = 0;
    uint32_t r_seen = 0, e_pub = 0xffffffffu;
    while (true) {
        // ---- claim the next published entry (lane 0): its tag and ray are read
        // before the claim (a claimed ring slot may be reused at once)
        uint32_t e = 0, slot = 0;
        RtF4 ro4{0, 0, 0, 0}, rd4{0, 0, 0, 0};
        int quit = 0;
        if (lane == 0) {
            WfCold &cs = WF_COLD(st);
            uint32_t *const reserved = cs.long_ctr, *const claimed = cs.long_ctr + 1, *const running = cs.long_ctr + 3;
            while (true) {
                const unsigned long long now = __builtin_amdgcn_s_memrealtime();
                ++n_idle;
                ++n_net;
                // (producers first: once they are all past their last hand-off,
                // `reserved` read after this acquire holds every entry.)  A finisher
                // that has not started is not waited for (WF_LONG_START_TRIPS below)
                const uint32_t fl = persist ? __hip_atomic_load(cs.fin_live, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
                const bool unstarted = persist && !(fl & WF_FIN_STARTED);
                const bool producing = persist && !unstarted && (fl & ~WF_FIN_STARTED) != 0u;
                const bool others = __hip_atomic_load(running, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u;
                const bool chain_open =
                    persist && __hip_atomic_load(cs.chain_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u;
                if (persist && !producing && !unstarted) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                e = __hip_atomic_load(claimed, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const uint32_t rw = __hip_atomic_load(reserved, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const bool closed = (rw & WF_LONG_CLOSED) != 0u;
                const uint32_t r = rw & ~WF_LONG_CLOSED;
                const bool flowing = r != r_seen;
                if (flowing) { // entries still flowing (to any wave): not idle
                    r_seen = r;
                    t_idle = now;
                    n_idle = 0;
                }
                if (flowing || producing || others) { // work may still come: a bounded wait
                    t_net = now;
                    n_net = 0;
                }
                // done once nothing can bring entries: the ring closed, or the call's finisher
                // past its last hand-off and no chain open (or its window over)
                const bool window_over = (now - t_idle > WF_LONG_CHAIN_IDLE || n_idle > WF_LONG_CHAIN_TRIPS) && !others;
                const bool done = persist && (closed || (!producing && !unstarted && (!chain_open || window_over)));
                if (cs.debug_quit) { // (tests: as if the net fired at once)
                    quit = 2;
                    break;
                }
                if (e < r) {
                    const uint32_t k = e % cs.long_cap;
                    const unsigned long long v =
                        __hip_atomic_load(cs.long_ent + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if ((uint32_t)(v >> 32) == e + 1u) { // published: acquire, read, then claim
                        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                        ro4 = ldf4(cs.long_ray + 2 * (size_t)k);
                        rd4 = ldf4(cs.long_ray + 2 * (size_t)k + 1);
                        slot = (uint32_t)v;
                        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                        uint32_t expect = e;
                        if (__hip_atomic_compare_exchange_strong(claimed, &expect, e + 1u, __ATOMIC_RELAXED,
                                                                 __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
                            __hip_atomic_fetch_add(running, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                            break;
                        }
                        continue; // another wave took it: try the next one
                    }
                    // reserved, its publication still in flight: wait for it (safety net: 1 s)
                    if (e != e_pub) {
                        e_pub = e;
                        t_pub = now;
                        n_pub = 0;
                    } else if (now - t_pub > WF_LONG_PUBLISH_WAIT || ++n_pub > WF_LONG_PUBLISH_TRIPS) {
                        quit = 2;
                        break;
                    }
                } else {
                    // nothing claimable.  Persistent: done once nothing can bring entries; slices: the
                    // final one once every entry is claimed, the others unless a path still runs.
                    if (persist ? done : (final_slice || !others)) {
                        quit = 1;
                        break;
                    }
                    // the call's finisher has not started: it may be dispatched only after this kernel
                    // ends (serialised dispatch).  After WF_LONG_START_TRIPS such trips close the ring —
                    // atomically with the reservations, so only while every entry is claimed — and
                    // leave: the finisher then keeps its deep paths
                    if (unstarted && !closed && ++n_start > WF_LONG_START_TRIPS) {
                        uint32_t x = r;
                        if (__hip_atomic_compare_exchange_strong(reserved, &x, r | WF_LONG_CLOSED, __ATOMIC_RELAXED,
                                                                 __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
                            atomicAdd(fr.dev_stats + RT_DEV_LONG_CLOSED, 1ull);
                            quit = 1;
                            break;
                        }
                        continue; // a reservation came in: serve it
                    }
                }
                if (now - t_net > WF_LONG_IDLE || n_net > WF_LONG_IDLE_TRIPS) { // safety net (see WF_LONG_IDLE)
                    quit = e < r ? 2 : 1;
                    break;
                }
                __builtin_amdgcn_s_sleep(16);
            }
            if (!quit) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            if (quit == 2) atomicAdd(fr.dev_stats + RT_DEV_LONG_QUIT, 1ull); // entries left unclaimed: stranded
        }
        // (lane 0's values, wave-uniform: readfirstlane — every lane is active here)
        if (__builtin_amdgcn_readfirstlane(quit)) break;
        e = (uint32_t)__builtin_amdgcn_readfirstlane((int)e);
        // ---- run the path (state in lane 0)
        PathRegs p;
        p.slot = 0;
        p.ro = p.rd = rt_v3(0, 0, 0);
        if (lane == 0) {
            load_regs(WF_COLD(st), fr, slot, p);
            p.ro = ld3(ro4);
            p.rd = ld3(rd4);
        }
        int want = 0; // after the loop: 0 the pixel's passes are done, 2 returned to the finishers
        uint32_t ret_e = 0;
        const unsigned long long t_claim = __builtin_amdgcn_s_memrealtime();
        uint32_t bounces = 0;
        while (true) {
            ++bounces;
            int hit = -1;
            float bx = 0.0f, by = 0.0f, bz = 0.0f;
            CoopRay r;
            coop_idle(r);
            if (lane == 0) {
                if (COUNT) c.v[RT_CNT_RAY]++;
                coop_begin(sc, r, p.ro, p.rd);
            }
            if (__shfl((int)r.live, 0)) {
                const Vec3D o = rt_v3(__shfl(r.o.x, 0), __shfl(r.o.y, 0), __shfl(r.o.z, 0));
                const Vec3D d = rt_v3(__shfl(r.d.x, 0), __shfl(r.d.y, 0), __shfl(r.d.z, 0));
                const float en = __shfl(r.entry, 0), ex = __shfl(r.exit_, 0);
                // bounded (bvh_trace.h trace_bvh, one ray per wave): the wave-wide s_min query, then the
                // bounded KD traversal run by the whole wave, its nodes fetched 64 at a time and its stack in LDS.  A query that outgrows its lists
                // is abandoned and counted, and the ray takes the wide KD traversal below, as do rays
                // the bound does not apply to (rt_bounded_ray)
                bool traced = false;
                bool certified = false;
                if (st.long_wide && rt_bounded_ray(o, d, sc.split_vals, sc.split_off)) {
                    float s_min = ex;
                    int tk = -1;
                    traced = wide_smin<COUNT>(sc, o, d, ex, wsm_lds(W.F, W.key, st.long_wide == 2), s_min, tk, c);
                    // the T* certificate (bvh_trace.h kd_certified) on the wave's one ray, every lane alike: where
                    // it holds the bounce needs no descent
                    if (traced && s_min < ex)
                        certified = kd_certified<COUNT>(sc, o, d, en, ex, s_min, tk, hit, bx, by, bz, c, lane == 0);
                    if (traced && s_min < ex && !certified) {
                        // (every lane: kd_bounded_wave)
                        LdsStack1 ks{reinterpret_cast<uint2 *>(W.mark)}; // (128 ints: WSM_KD_STACK entries)
                        const int tstar = tk >= 0 ? (int)sc.bvh_bary[tk].tri : -1;
                        hit = kd_bounded_wave<COUNT>(sc, o, d, en, ex, s_min, tstar, bx, by, bz, ks,
                                                     reinterpret_cast<unsigned long long *>(W.F), c);
                    }
                    if (!traced && lane == 0) atomicAdd(fr.dev_stats + RT_DEV_WIDE_OVERFLOW, 1ull);
                }
                if (!traced) {
                    // entered at the origin's grid cell (kd_origin_frontier), else from the root
                    const int nf = !COUNT && sc.kd_grid > 0 ? kd_origin_frontier(sc, o, d, en, ex, W) : 0;
                    if (nf > 0) wide_trace_from<COUNT>(sc, o, d, nf, W, lane == 0, hit, bx, by, bz, c);
                    else wide_trace<COUNT>(sc, o, d, en, ex, W, lane == 0, hit, bx, by, bz, c);
                }
                if (COUNT && lane == 0 && hit >= 0 && !certified) c.cert[1]++; // (found by a KD descent)
            }
            want = 0;
            if (lane == 0) {
                want = shade_step<COUNT>(sc, fr, WF_COLD_CAM(cam), p, hit, bx, by, bz, limit, c) ? 1 : 0;
                if (!want && st.long_return) {
                    // the pixel's passes are done: run the passes chained calls owe it, or
                    // release it — its state stored and released before the word says so
                    WfCold &cs = WF_COLD(st);
                    while (true) {
                        store_regs(cs, fr, p);
                        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
                        uint32_t x = RT_PX_OUT;
                        if (__hip_atomic_compare_exchange_strong(cs.pxo + p.slot, &x, RT_PX_LONGDONE, __ATOMIC_RELAXED,
                                                                 __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
                            break;
                        x = __hip_atomic_exchange(cs.pxo + p.slot, RT_PX_OUT, __ATOMIC_RELAXED,
                                                  __HIP_MEMORY_SCOPE_AGENT);
                        p.passes_left = (int)(x & RT_PX_PASSES);
                        if (x & RT_PX_PASSES) { // (RtDeviations: owed passes, run here in the pixel's order)
                            atomicAdd(fr.dev_stats + RT_DEV_OWED_PIXELS, 1ull);
                            atomicAdd(fr.dev_stats + RT_DEV_OWED_PASSES, (unsigned long long)(x & RT_PX_PASSES));
                        }
                        const Vec3D fb = fr.fb[p.slot];
                        const float sq = fr.sq[p.slot];
                        const int count = fr.count[p.slot];
                        if (start_sample<COUNT>(fr, WF_COLD_CAM(cam), (int)p.slot, p.passes_left, p.rng, fb, sq, count, p.ro, p.rd,
                                                c)) { // as shade_step's next pass
                            p.T = rt_v3(1.0f, 1.0f, 1.0f);
                            p.L = rt_v3(0.0f, 0.0f, 0.0f);
                            p.inside = false;
                            p.prev_type = PRIMARY;
                            p.depth = 1;
                            p.shadow = false;
                            want = 1;
                            break;
                        }
                    }
                }
                // return mode: the deep sample is over once the pixel's next one starts (depth 1);
                // the pixel goes back to the finishers if one is still alive to take it.  While a
                // chain is open: always — this call's, the next call's or the chain's drain
                // finisher takes it (a finisher in its tail takes none: a returned pixel's whole
                // remaining chain would hold up the call's end and the next call's start).  The
                // drain finisher lingers (WF_FIN_LINGER) while a pixel is out, so a return
                // reserved just as its clear of the flag lands is still taken.
                if (want && st.long_return && p.depth == 1 && !p.shadow) {
                    WfCold &cs = WF_COLD(st);
                    unsigned long long *const ret_word = reinterpret_cast<unsigned long long *>(cs.ret_ctr);
                    if (cs.linger == 0ull &&
                        __hip_atomic_load(cs.chain_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) {
                        want = 2;
                        ret_e = (uint32_t)__hip_atomic_fetch_add(ret_word, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    }
                    unsigned long long w = __hip_atomic_load(ret_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    while (want != 2 && (w >> 32) != 0ull) {
                        if (__hip_atomic_compare_exchange_strong(ret_word, &w, w + 1ull, __ATOMIC_RELAXED,
                                                                 __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
                            want = 2;
                            ret_e = (uint32_t)w;
                            break;
                        }
                    }
                }
            }
            want = __builtin_amdgcn_readfirstlane(want);
            if (want != 1) break;
        }
        if (lane == 0) {
            WfCold &cs = WF_COLD(st);
            if (cs.long_log && e < 65535u) {
                unsigned long long *L = cs.long_log + 4 + 4 * (size_t)e;
                L[0] = t_claim;
                L[1] = __builtin_amdgcn_s_memrealtime();
                L[2] = bounces;
                L[3] = p.slot;
            }
            if (want == 2) { // back to the finishers: its state and next ray, then its ring entry
                store_regs(cs, fr, p);
                cs.ro[p.slot] = p.ro;
                cs.cont[p.slot] = p.rd;
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __hip_atomic_store(cs.ret_ring + ret_e % cs.long_cap, ((unsigned long long)(ret_e + 1u) << 32) | p.slot,
                                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            } else if (st.long_return) { // done and released above (its state may already be another's)
                __hip_atomic_fetch_sub(cs.ret_ctr + 3, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            } else {
                store_regs(cs, fr, p);
            }
            __hip_atomic_fetch_sub(cs.long_ctr + 3, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        t_idle = __builtin_amdgcn_s_memrealtime();
        n_idle = 0;
    }
    if (COUNT) {
        flush_counters(c, fr.counters);
        flush_cert_counters(c, fr.dev_stats);
    }
}
