// wf_queue_kernels.h — the queue mode's kernels: wf_start and the trace launches (wf_trace, wf_trace_bvh_dyn,
// wf_trace_dyn, wf_trace_coop).
// A part of wavefront.hip's translation unit (included there, once, in the order wf_state.h,
// wf_queue_kernels.h, wf_shade.h, wf_finish_kernels.h, wf_long.h): not for use elsewhere.
#pragma once

namespace {

// start the pixel's next pass(es): adaptive test, camera ray.  Returns true
// (and the ray) when a sample starts.
template <bool COUNT>
__device__ __forceinline__ bool start_sample(const RtDevFrame &fr, const RtDevCamera &cam, int slot, int &passes_left,
                                             uint32_t &rng, Vec3D fb, float sq, int count, Vec3D &ro, Vec3D &rd,
                                             Cnt &c)
{
    while (passes_left > 0) {
        --passes_left;
        if (!adaptive_run(fr, fb, sq, count)) {
            if (COUNT) c.v[RT_CNT_SKIP]++;
            continue;
        }
        camera_ray(fr, cam, slot % fr.width, slot / fr.width, rng, ro, rd);
        if (COUNT) c.v[RT_CNT_SAMPLE]++;
        return true;
    }
    return false;
}

// ray e's 16-byte record in hits[]: the triangle and the hit's barycentrics, or a miss (miss_record)
__device__ __forceinline__ void store_hit(const WfState &st, uint32_t e, int tri, float bx, float by, float bz)
{
    *reinterpret_cast<float4 *>(st.hits + e) = make_float4(__int_as_float(tri), bx, by, bz);
}
__device__ __forceinline__ void store_miss(const WfState &st, uint32_t e)
{
    *reinterpret_cast<float4 *>(st.hits + e) = miss_record();
}

} // namespace

template <bool COUNT>
__global__ void __launch_bounds__(WF_BLOCK) wf_start(RtDevFrame fr, RtDevCamera cam, WfState st, int pipe,
                                                     int npipes)
{
    Cnt c;
    if (COUNT) c.zero();
    const int n = fr.width * fr.height;
    const int tile = xcd_tile(blockIdx.x, gridDim.x);
    if (tile % npipes != pipe) return; // another pipeline's 16x16 tile (block-uniform)
    const int tiles_x = (fr.width + 15) / 16;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int x = (tile % tiles_x) * 16 + (wave & 1) * 8 + (lane & 7);
    const int y = (tile / tiles_x) * 16 + (wave >> 1) * 8 + (lane >> 3);
    const bool valid = x < fr.width && y < fr.height && rt_row_owned(fr, y);
    const int slot = valid ? y * fr.width + x : 0;
    bool want = false;
    Vec3D ro = rt_v3(0, 0, 0), rd = rt_v3(0, 0, 0);
    if (valid && slot < n) {
        Vec3D fb = rt_v3(0.0f, 0.0f, 0.0f);
        float sq = 0.0f;
        int count = 0;
        if (fr.reset) {
            fr.fb[slot] = fb;
            fr.sq[slot] = sq;
            fr.count[slot] = count;
        } else {
            fb = fr.fb[slot];
            sq = fr.sq[slot];
            count = fr.count[slot];
        }
        int passes_left = fr.passes;
        uint32_t rng = fr.rng[slot];
        want = start_sample<COUNT>(fr, cam, slot, passes_left, rng, fb, sq, count, ro, rd, c);
        fr.rng[slot] = rng;
        st.passes_left[slot] = passes_left;
        st.flags[slot] = 1u << 8; // depth 1 (first extension ray), prev PRIMARY
        st.T[slot] = rt_v3(1.0f, 1.0f, 1.0f);
        st.L[slot] = rt_v3(0.0f, 0.0f, 0.0f);
        st.ro[slot] = ro;
        st.cont[slot] = rd;
    }
    const uint32_t e = enqueue_ray(st, 0, want, ro, rd);
    if (want) st.e_ext[slot] = e;
    enqueue_path(st, 0, want, (uint32_t)slot);
    if (COUNT) flush_counters(c, fr.counters);
}

template <bool COUNT>
__global__ void __launch_bounds__(WF_BLOCK) wf_trace(RtDevScene sc, WfState st, int q, unsigned long long *counters)
{
    __shared__ uint32_t s_node[WF_LDS_STACK * WF_BLOCK];
    __shared__ float s_entry[WF_LDS_STACK * WF_BLOCK];
    const int tid = threadIdx.x;
    const int gtid = blockIdx.x * WF_BLOCK + tid;
    Stack<WF_LDS_STACK> stk{s_node + tid, s_entry + tid, WF_BLOCK, st.spill + gtid, st.spill_threads};
    Cnt c;
    if (COUNT) c.zero();
    const uint32_t n = st.counts[q];
    const RtF4 *rays = st.q_ray[q];
    for (uint32_t base = blockIdx.x * WF_BLOCK; base < n; base += gridDim.x * WF_BLOCK) {
        const uint32_t e = base + tid;
        if (e < n) {
            const RtF4 o4 = ldf4(rays + 2 * (size_t)e), d4 = ldf4(rays + 2 * (size_t)e + 1);
            float bx = 0.0f, by = 0.0f, bz = 0.0f;
            const int hit = trace<COUNT>(sc, ld3(o4), ld3(d4), bx, by, bz, stk, c);
            store_hit(st, e, hit, bx, by, bz);
        }
    }
    if (COUNT) flush_counters(c, counters);
}

// trace_bvh (bvh_trace.h) with dynamic ray fetch: every lane runs its own ray
// through the same steps — the s_min query over the 4-wide BVH, then the
// bounded KD phase — but a round advances each lane by at most `cap` node
// steps of its current phase and one leaf, and a lane whose ray is done takes
// the next queued ray at the start of the next round (Aila & Laine's
// persistent while-while with per-lane refill), so a wave is not held for its
// slowest ray.  Same per-ray arithmetic and visiting order as trace_bvh: the
// same hits, bit for bit.  (Rays that lie in a KD split plane — zero direction
// components — take the plain KD traversal, as in trace_bvh: s_min = -inf.)
#ifndef WF_DYN_WAVES
#define WF_DYN_WAVES 6
#endif
#ifndef WF_BVH_DYN_CAP
#define WF_BVH_DYN_CAP 8 // node steps per phase per round
#endif
template <bool COUNT>
__global__ void __launch_bounds__(WF_BLOCK, WF_DYN_WAVES) wf_trace_bvh_dyn(RtDevScene sc, WfState st, int q,
                                                                          unsigned long long *counters, int cap)
{
    Cnt c;
    if (COUNT) c.zero();
    __shared__ uint32_t s_node[WF_BVH_LDS * WF_BLOCK];
    __shared__ float s_entry[WF_BVH_LDS * WF_BLOCK];
    const int tid = threadIdx.x;
    const int gtid = blockIdx.x * WF_BLOCK + tid;
    Stack<WF_BVH_LDS> stk{s_node + tid, s_entry + tid, WF_BLOCK, st.spill + gtid, st.spill_threads};
    const uint32_t n = st.counts[q];
    const RtF4 *rays = st.q_ray[q];
    uint32_t *fetch = st.counts + 2 + q;
    const int lane = __lane_id();
    // per lane: 0 no ray, 1 s_min query (cur: BVH4 reference), 2 KD phase (node, nd: its words once loaded)
    int phase = 0;
    bool exhausted = false;
    uint32_t e = 0, cur = 0, node = 0;
    uint2 nd = make_uint2(0u, 0u);
    bool nd_ok = false; // nd holds node's words
    int sp = 0;
    Vec3D o = rt_v3(0, 0, 0), d = rt_v3(0, 0, 0);
    RtSlab sl{rt_v3(0, 0, 0), rt_v3(0, 0, 0), rt_v3(0, 0, 0)};
    float best = 0.0f, entry = 0.0f, exit_ = 0.0f, root_exit = 0.0f, s_min = 0.0f;
    while (true) {
        // ---- refill: lanes without a ray take the next queued one
        if (phase == 0 && !exhausted) {
            e = wave_next_index(fetch, lane);
            if (e >= n) {
                exhausted = true;
            } else {
                o = ld3(ldf4(rays + 2 * (size_t)e));
                d = ld3(ldf4(rays + 2 * (size_t)e + 1));
                if (COUNT) c.v[RT_CNT_RAY]++;
                if (!bbox_hit(sc, o, d, entry, exit_)) {
                    store_miss(st, e);
                } else {
                    root_exit = exit_;
                    sp = 0;
                    if (rt_bounded_ray(o, d, sc.split_vals, sc.split_off)) {
                        phase = 1;
                        sl = rt_slab(o, d, rt_ray_margin(o.x, o.y, o.z, sc.bvh_scale));
                        best = exit_;
                        cur = 0;
                    } else {
                        phase = 2; // the plain KD traversal
                        s_min = -INFINITY;
                        node = 0;
                        nd_ok = false;
                    }
                }
            }
        }
        if (!__any(phase != 0)) {
            if (__all(exhausted)) break;
            continue;
        }
        // ---- s_min query: up to `cap` inner nodes, then a leaf (bvh4_bound)
        for (int i = 0; i < cap; ++i) {
            const bool step = phase == 1 && !(cur & RT_BVH_LEAF);
            if (!__any(step)) break;
            if (step) {
                if (COUNT) c.v[RT_CNT_B_BVH_NODE]++;
                const uint32_t next = bvh4_children(sc, cur, sl, best, stk, sp);
                cur = next != RT_BVH_EMPTY ? next : bvh_pop(stk, sp, best);
            }
        }
        // (cur == RT_BVH_EMPTY carries the leaf bit: such a lane is done with the query)
        const bool bleaf = phase == 1 && (cur & RT_BVH_LEAF) && cur != RT_BVH_EMPTY;
        if (__any(bleaf) && bleaf) {
            const uint32_t first = (cur & ~RT_BVH_LEAF) >> 3, end = first + (cur & 7u) + 1u;
            if (COUNT) c.v[RT_CNT_B_BVH_TRI] += end - first;
            float bx, by, bz;
            (void)leaf_scan<COUNT>(sc.bvh_a, sc.bvh_bary, first, end, o, d, best, bx, by, bz, c);
            cur = bvh_pop(stk, sp, best);
        }
        if (phase == 1 && cur == RT_BVH_EMPTY) { // the query is over: s_min, then the KD phase (or a miss)
            s_min = best;
            if (!(s_min < root_exit)) {
                store_miss(st, e);
                phase = 0;
            } else {
                phase = 2;
                node = 0;
                nd_ok = false;
                sp = 0;
                exit_ = root_exit; // (entry: the scene box's, unchanged since the refill)
            }
        }
        // ---- KD phase (trace_bvh's): up to `cap` node fetches, then the leaf
        for (int i = 0; i < cap; ++i) {
            const bool step = phase == 2 && !(nd_ok && (nd.y & 3u) == RT_LEAF_TAG);
            if (!__any(step)) break;
            if (step) {
                if (nd_ok) { // an inner node: the reference's split step
                    const float dax = kd_axis(nd.y & 3u, d);
                    kd_split_step<KD_DEVICE_DIV, KD_BOUNDED>(nd, kd_axis(nd.y & 3u, o), dax, rt_recip_guard(dax), s_min,
                                                             node, entry, exit_, sp, stk);
                }
                nd = ldc_u2(sc.nodes + 2 * (size_t)node);
                nd_ok = true;
                if (COUNT) c.v[RT_CNT_NODE]++;
            }
        }
        const bool kleaf = phase == 2 && nd_ok && (nd.y & 3u) == RT_LEAF_TAG;
        if (__any(kleaf) && kleaf) {
            const uint32_t count = nd.y >> 2;
            int best_tri = -1;
            float bx = 0.0f, by = 0.0f, bz = 0.0f;
            if (count > 0 && exit_ > s_min) { // trace_leaf_node (:115-172): closest starts at the leaf's exit
                float smallest = exit_;
                if (COUNT) c.v[RT_CNT_TRI] += count;
                const int be = leaf_scan<COUNT>(sc.isect_a, sc.isect_bary, nd.x, nd.x + count, o, d, smallest, bx, by,
                                                bz, c);
                best_tri = be >= 0 ? (int)ldc_u2(&sc.isect_bary[be].rd).y : -1;
            }
            if (best_tri >= 0) {
                if (COUNT) c.v[RT_CNT_HIT]++;
                store_hit(st, e, best_tri, bx, by, bz);
                phase = 0;
            } else if (sp == 0) {
                store_miss(st, e);
                phase = 0;
            } else {
                kd_pop(stk, sp, root_exit, node, entry, exit_);
                nd_ok = false;
            }
        }
    }
    if (COUNT) flush_counters(c, counters);
}

// Persistent trace with dynamic ray fetch: every lane runs rays one leaf at a
// time; a lane whose ray is done writes its hit and takes the next queued ray
// at the next leaf boundary (one wave-aggregated atomic), so a wave is never
// held by its slowest ray.  The per-ray arithmetic is trace()'s own: the same split step, leaf scan and pop
// (rt_kernels.h kd_split_step, leaf_scan_pairs, kd_pop).
template <bool COUNT>
__global__ void __launch_bounds__(WF_BLOCK) wf_trace_dyn(RtDevScene sc, WfState st, int q,
                                                         unsigned long long *counters)
{
    __shared__ uint32_t s_node[WF_LDS_STACK * WF_BLOCK];
    __shared__ float s_entry[WF_LDS_STACK * WF_BLOCK];
    const int tid = threadIdx.x;
    const int gtid = blockIdx.x * WF_BLOCK + tid;
    Stack<WF_LDS_STACK> stk{s_node + tid, s_entry + tid, WF_BLOCK, st.spill + gtid, st.spill_threads};
    Cnt c;
    if (COUNT) c.zero();
    const uint32_t n = st.counts[q];
    const RtF4 *rays = st.q_ray[q];
    uint32_t *fetch = st.counts + 2 + q;
    const int lane = __lane_id();

    bool live = false, exhausted = false;
    uint32_t e = 0, node = 0;
    int sp = 0;
    Vec3D o = rt_v3(0, 0, 0), d = rt_v3(0, 0, 0);
    float entry = 0.0f, exit_ = 0.0f, root_exit = 0.0f;
    while (true) {
        // ---- refill idle lanes
        if (!live && !exhausted) {
            e = wave_next_index(fetch, lane);
            if (e >= n) {
                exhausted = true;
            } else {
                o = ld3(ldf4(rays + 2 * (size_t)e));
                d = ld3(ldf4(rays + 2 * (size_t)e + 1));
                if (COUNT) c.v[RT_CNT_RAY]++;
                if (bbox_hit(sc, o, d, entry, exit_)) {
                    root_exit = exit_;
                    node = 0;
                    sp = 0;
                    live = true;
                } else {
                    store_miss(st, e);
                }
            }
        }
        if (!__any(live)) {
            if (__all(exhausted)) break;
            continue;
        }
        if (!live) continue;
        // ---- descend to a leaf (rt/trace_ray.cuh:273-306)
        uint2 nd = *reinterpret_cast<const uint2 *>(sc.nodes + 2 * (size_t)node);
        if (COUNT) c.v[RT_CNT_NODE]++;
        while ((nd.y & 3u) != RT_LEAF_TAG) {
            const uint32_t axis = nd.y & 3u;
            const bool pushed = kd_split_step<KD_IEEE_DIV, KD_PLAIN>(nd, kd_axis(axis, o), kd_axis(axis, d), 0.0f, 0.0f,
                                                                     node, entry, exit_, sp, stk);
            if (COUNT && pushed && sp - 1 >= RT_REF_STACK) c.v[RT_CNT_DEEP_PUSH]++;
            nd = *reinterpret_cast<const uint2 *>(sc.nodes + 2 * (size_t)node);
            if (COUNT) c.v[RT_CNT_NODE]++;
        }
        // ---- leaf (rt/trace_ray.cuh:115-172)
        const uint32_t count = nd.y >> 2;
        float bx = 0.0f, by = 0.0f, bz = 0.0f;
        const int best = count > 0 ? leaf_scan_pairs<COUNT>(sc, nd.x, nd.x + count, o, d, exit_, bx, by, bz, c) : -1;
        if (best >= 0) {
            if (COUNT) c.v[RT_CNT_HIT]++;
            store_hit(st, e, best, bx, by, bz);
            live = false;
        } else if (sp == 0) {
            store_miss(st, e);
            live = false;
        } else {
            kd_pop(stk, sp, root_exit, node, entry, exit_);
        }
    }
    if (COUNT) flush_counters(c, counters);
}

#include "coop_trace.h"
#include "wide_bvh.h"

// Wave-cooperative trace with dynamic ray fetch (coop_trace.h): lanes whose
// ray finished take the next queued ray at the next round; descents are
// capped at `cap` node fetches per round and the leaf test waits for
// `postpone` pending lanes.
template <bool COUNT>
__global__ void __launch_bounds__(WF_TBLOCK, WF_TRACE_WAVES) wf_trace_coop(RtDevScene sc, WfState st, int q,
                                                          unsigned long long *counters, int cap, int postpone,
                                                          int wide_lanes, unsigned long long *timeline)
{
    // debug timeline (RtOptions.wave_times_device): s_memrealtime of the
    // launch's first wave start, first queue exhaustion, last wave end
    // (stored as ~t so that all three are atomicMin)
    if (timeline && __lane_id() == 0) atomicMin(timeline, __builtin_amdgcn_s_memrealtime());
    __shared__ uint32_t s_node[WF_LDS_STACK * WF_TBLOCK];
    __shared__ float s_entry[WF_LDS_STACK * WF_TBLOCK];
    __shared__ unsigned long long s_key[WF_TBLOCK];
    __shared__ CoopCand s_list[(WF_TBLOCK / 64) * WF_COOP_LIST];
    __shared__ int s_mark[2 * WF_TBLOCK]; // 128 per wave: chunk_owner marks + junk slots
    const int tid = threadIdx.x;
    const int gtid = blockIdx.x * WF_TBLOCK + tid;
    const int lane = __lane_id();
    const int wave = tid >> 6;
    Stack<WF_LDS_STACK> stk{s_node + tid, s_entry + tid, WF_TBLOCK, st.spill + gtid, st.spill_threads};
    unsigned long long *wkey = s_key + wave * 64;
    CoopCand *list = s_list + wave * WF_COOP_LIST;
    const CoopLds w{wkey, list, s_mark + wave * 128};
    Cnt c;
    if (COUNT) c.zero();
    const uint32_t n = st.counts[q];
    const RtF4 *rays = st.q_ray[q];
    uint32_t *fetch = st.counts + 2 + q;

    CoopRay r;
    coop_idle(r);
    bool exhausted = false;
    uint32_t e = 0;
    while (true) {
        const unsigned long long tf = COUNT ? __builtin_amdgcn_s_memtime() : 0ull;
        // ---- refill idle lanes (dynamic ray fetch)
        if (!r.live && !exhausted) {
            e = wave_next_index(fetch, lane);
            if (e >= n) {
                exhausted = true;
                if (timeline && e == n) atomicMin(timeline + 1, __builtin_amdgcn_s_memrealtime());
            } else {
                if (COUNT) c.v[RT_CNT_RAY]++;
                if (!coop_begin(sc, r, ld3(ldf4(rays + 2 * (size_t)e)), ld3(ldf4(rays + 2 * (size_t)e + 1))))
                    store_miss(st, e);
            }
        }
        if (COUNT && lane == 0) c.v[RT_CNT_T_FETCH] += __builtin_amdgcn_s_memtime() - tf;
        if (WF_TAIL_PRIO > 0 && __any(exhausted)) __builtin_amdgcn_s_setprio(WF_TAIL_PRIO); // the launch's tail
        if (!__any(r.live)) {
            if (__all(exhausted)) break;
            continue;
        }
        int tri = -1;
        float bx = 0.0f, by = 0.0f, bz = 0.0f;
        // the launch's tail: the queue is empty and few rays are left in this
        // wave — leave the loop and finish them wide (below)
        if (wide_lanes > 0 && __any(exhausted) && __popcll(__ballot(r.live)) <= wide_lanes) break;
        if (coop_round<COUNT>(sc, r, stk, w, cap, postpone, tri, bx, by, bz, c))
            store_hit(st, e, tri, bx, by, bz);
    }
    // finish the wave's remaining rays one at a time with all 64 lanes
    // (wide_resume) instead of letting the longest run alone at one lane's pace
    const unsigned long long lm = __ballot(r.live);
    if (lm) {
        const WideLds W{reinterpret_cast<WideItem *>(list),
                        WF_COOP_LIST * (int)sizeof(CoopCand) / (int)sizeof(WideItem), wkey,
                        reinterpret_cast<float *>(wkey + 1), w.mark};
        for (unsigned long long mm = lm; mm; mm &= mm - 1) {
            const int owner = __ffsll((long long)mm) - 1;
            const int ot = wave * 64 + owner;
            const Stack<WF_LDS_STACK> so{s_node + ot, s_entry + ot, WF_TBLOCK, st.spill + blockIdx.x * WF_TBLOCK + ot,
                                         st.spill_threads};
            int tri = -1;
            float bx = 0.0f, by = 0.0f, bz = 0.0f;
            wide_resume<COUNT>(sc, r, owner, so, W, tri, bx, by, bz, c);
            if (lane == owner) store_hit(st, e, tri, bx, by, bz);
        }
    }
    if (timeline && lane == 0) atomicMin(timeline + 2, ~__builtin_amdgcn_s_memrealtime());
    if (COUNT) flush_counters(c, counters);
}
