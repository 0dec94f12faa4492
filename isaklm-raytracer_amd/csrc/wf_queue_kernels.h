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
            *reinterpret_cast<float4 *>(st.hits + e) = make_float4(__int_as_float(hit), bx, by, bz);
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
        const bool need = phase == 0 && !exhausted;
        const unsigned long long mm = __ballot(need);
        if (mm) {
            const int leader = __ffsll((long long)mm) - 1;
            uint32_t base = 0;
            if (lane == leader) base = atomicAdd(fetch, (uint32_t)__popcll(mm));
            base = __shfl(base, leader);
            if (need) {
                e = base + (uint32_t)__popcll(mm & ((1ull << lane) - 1ull));
                if (e >= n) {
                    exhausted = true;
                } else {
                    o = ld3(ldf4(rays + 2 * (size_t)e));
                    d = ld3(ldf4(rays + 2 * (size_t)e + 1));
                    if (COUNT) c.v[RT_CNT_RAY]++;
                    if (!bbox_hit(sc, o, d, entry, exit_)) {
                        *reinterpret_cast<float4 *>(st.hits + e) = miss_record();
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
                if (next != RT_BVH_EMPTY) {
                    cur = next;
                } else { // pop the next subtree that may still hold a smaller s
                    cur = RT_BVH_EMPTY;
                    while (sp > 0) {
                        uint32_t nn;
                        float tn;
                        stk.get(--sp, nn, tn);
                        if (tn <= best) {
                            cur = nn;
                            break;
                        }
                    }
                }
            }
        }
        // (cur == RT_BVH_EMPTY carries the leaf bit: such a lane is done with the query)
        const bool bleaf = phase == 1 && (cur & RT_BVH_LEAF) && cur != RT_BVH_EMPTY;
        if (__any(bleaf) && bleaf) {
            const uint32_t first = (cur & ~RT_BVH_LEAF) >> 3, end = first + (cur & 7u) + 1u;
            if (COUNT) c.v[RT_CNT_B_BVH_TRI] += end - first;
            float bx, by, bz;
            (void)leaf_scan<COUNT>(sc.bvh_a, sc.bvh_bary, first, end, o, d, best, bx, by, bz, c);
            cur = RT_BVH_EMPTY;
            while (sp > 0) {
                uint32_t nn;
                float tn;
                stk.get(--sp, nn, tn);
                if (tn <= best) {
                    cur = nn;
                    break;
                }
            }
        }
        if (phase == 1 && cur == RT_BVH_EMPTY) { // the query is over: s_min, then the KD phase (or a miss)
            s_min = best;
            if (!(s_min < root_exit)) {
                *reinterpret_cast<float4 *>(st.hits + e) = miss_record();
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
                    const uint32_t axis = nd.y & 3u;
                    const float split = as_float(nd.x);
                    const float oax = axis == 0 ? o.x : (axis == 1 ? o.y : o.z);
                    const float dax = axis == 0 ? d.x : (axis == 1 ? d.y : d.z);
                    const float yax = rt_recip_guard(dax);
                    uint32_t near_c = node + 1, far_c = nd.y >> 2;
                    if (oax >= split) { // ray_behind_plane (rt/trace_ray.cuh:174-188)
                        near_c = nd.y >> 2;
                        far_c = node + 1;
                    }
                    const float t = rt_div_by(split - oax, dax, yax); // intersect_plane (:190-210)
                    if (t >= exit_ || t < 0) {
                        node = near_c;
                    } else if (t <= entry) {
                        node = far_c;
                    } else if (t <= s_min) { // the near side holds no hit: its leaves' exits are <= t
                        node = far_c;
                        entry = t;
                    } else {
                        stk.put(sp++, far_c, t);
                        node = near_c;
                        exit_ = t;
                    }
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
                *reinterpret_cast<float4 *>(st.hits + e) = make_float4(__int_as_float(best_tri), bx, by, bz);
                phase = 0;
            } else if (sp == 0) {
                *reinterpret_cast<float4 *>(st.hits + e) = miss_record();
                phase = 0;
            } else {
                --sp;
                node = stk.node_at(sp);
                entry = stk.entry_at(sp);
                exit_ = sp > 0 ? stk.entry_at(sp - 1) : root_exit;
                nd_ok = false;
            }
        }
    }
    if (COUNT) flush_counters(c, counters);
}

// Persistent trace with dynamic ray fetch: every lane runs rays one leaf at a
// time; a lane whose ray is done writes its hit and takes the next queued ray
// at the next leaf boundary (one wave-aggregated atomic), so a wave is never
// held by its slowest ray.  Same per-ray arithmetic as trace().
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
        const bool need = !live && !exhausted;
        const unsigned long long m = __ballot(need);
        if (m) {
            const int leader = __ffsll((long long)m) - 1;
            uint32_t base = 0;
            if (lane == leader) base = atomicAdd(fetch, (uint32_t)__popcll(m));
            base = __shfl(base, leader);
            if (need) {
                e = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
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
                        *reinterpret_cast<float4 *>(st.hits + e) = miss_record();
                    }
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
            const float split = as_float(nd.x);
            const float oax = axis == 0 ? o.x : (axis == 1 ? o.y : o.z);
            const float dax = axis == 0 ? d.x : (axis == 1 ? d.y : d.z);
            uint32_t near_c = node + 1, far_c = nd.y >> 2;
            if (oax >= split) {
                near_c = nd.y >> 2;
                far_c = node + 1;
            }
            const float t = (split - oax) / dax;
            if (t >= exit_ || t < 0) {
                node = near_c;
            } else if (t <= entry) {
                node = far_c;
            } else {
                if (COUNT && sp >= RT_REF_STACK) c.v[RT_CNT_DEEP_PUSH]++;
                stk.put(sp, far_c, t);
                ++sp;
                node = near_c;
                exit_ = t;
            }
            nd = *reinterpret_cast<const uint2 *>(sc.nodes + 2 * (size_t)node);
            if (COUNT) c.v[RT_CNT_NODE]++;
        }
        // ---- leaf (rt/trace_ray.cuh:115-172)
        const int count = (int)(nd.y >> 2);
        int best = -1;
        float bx = 0.0f, by = 0.0f, bz = 0.0f;
        if (count > 0) {
            const uint32_t e0 = nd.x, e1 = nd.x + (uint32_t)count;
            float smallest = exit_;
            for (uint32_t k = e0; k < e1; k += 2) {
                const bool two = k + 1 < e1;
                if (COUNT) c.v[RT_CNT_TRI] += two ? 2 : 1;
                const RtF4 A0 = ldf4(sc.isect_a + k);
                const RtF4 A1 = ldf4(sc.isect_a + (two ? k + 1 : k));
                const float dn0 = d.x * A0.x + d.y * A0.y + d.z * A0.z;
                const float dn1 = d.x * A1.x + d.y * A1.y + d.z * A1.z;
                const float s0 = (A0.w - (o.x * A0.x + o.y * A0.y + o.z * A0.z)) / dn0;
                const float s1 = (A1.w - (o.x * A1.x + o.y * A1.y + o.z * A1.z)) / dn1;
                const bool p0 = dn0 != 0 && s0 >= 0.00001f && s0 < smallest;
                const bool p1 = two && dn1 != 0 && s1 >= 0.00001f && s1 < smallest;
                RtF4 B0, C0, D0, B1, C1, D1;
                uint2 R0, R1;
                if (p0) {
                    B0 = ldf4(&sc.isect_bary[k].b);
                    C0 = ldf4(&sc.isect_bary[k].c);
                    D0 = ldf4(&sc.isect_bary[k].d);
                    R0 = *reinterpret_cast<const uint2 *>(&sc.isect_bary[k].rd);
                }
                if (p1) {
                    B1 = ldf4(&sc.isect_bary[k + 1].b);
                    C1 = ldf4(&sc.isect_bary[k + 1].c);
                    D1 = ldf4(&sc.isect_bary[k + 1].d);
                    R1 = *reinterpret_cast<const uint2 *>(&sc.isect_bary[k + 1].rd);
                }
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const bool p = j == 0 ? p0 : p1;
                    const float s = j == 0 ? s0 : s1;
                    if (!p || !(s < smallest)) continue;
                    const RtF4 B = j == 0 ? B0 : B1, C = j == 0 ? C0 : C1, D = j == 0 ? D0 : D1;
                    const uint2 R = j == 0 ? R0 : R1;
                    const float rd = as_float(R.x);
                    const float px = o.x + d.x * s, py = o.y + d.y * s, pz = o.z + d.z * s;
                    const float v2x = px - B.x, v2y = py - B.y, v2z = pz - B.z;
                    const float d20 = v2x * C.x + v2y * C.y + v2z * C.z;
                    const float d21 = v2x * D.x + v2y * D.y + v2z * D.z;
                    const float cy = (D.w * d20 - C.w * d21) * rd;
                    const float cz = (B.w * d21 - C.w * d20) * rd;
                    const float cx = 1.0f - cy - cz;
                    if (rt_bary_inside(cx, cy, cz)) {
                        smallest = s;
                        best = (int)R.y;
                        bx = cx;
                        by = cy;
                        bz = cz;
                    }
                }
            }
        }
        if (best >= 0) {
            if (COUNT) c.v[RT_CNT_HIT]++;
            *reinterpret_cast<float4 *>(st.hits + e) = make_float4(__int_as_float(best), bx, by, bz);
            live = false;
        } else if (sp == 0) {
            *reinterpret_cast<float4 *>(st.hits + e) = miss_record();
            live = false;
        } else {
            --sp;
            node = stk.node_at(sp);
            entry = stk.entry_at(sp);
            exit_ = sp > 0 ? stk.entry_at(sp - 1) : root_exit;
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
        const bool need = !r.live && !exhausted;
        const unsigned long long m = __ballot(need);
        if (m) {
            const int leader = __ffsll((long long)m) - 1;
            uint32_t base = 0;
            if (lane == leader) base = atomicAdd(fetch, (uint32_t)__popcll(m));
            base = __shfl(base, leader);
            if (need) {
                e = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
                if (e >= n) {
                    exhausted = true;
                    if (timeline && e == n) atomicMin(timeline + 1, __builtin_amdgcn_s_memrealtime());
                } else {
                    if (COUNT) c.v[RT_CNT_RAY]++;
                    if (!coop_begin(sc, r, ld3(ldf4(rays + 2 * (size_t)e)), ld3(ldf4(rays + 2 * (size_t)e + 1))))
                        *reinterpret_cast<float4 *>(st.hits + e) = miss_record();
                }
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
            *reinterpret_cast<float4 *>(st.hits + e) = make_float4(__int_as_float(tri), bx, by, bz);
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
            if (lane == owner) *reinterpret_cast<float4 *>(st.hits + e) = make_float4(__int_as_float(tri), bx, by, bz);
        }
    }
    if (timeline && lane == 0) atomicMin(timeline + 2, ~__builtin_amdgcn_s_memrealtime());
    if (COUNT) flush_counters(c, counters);
}
