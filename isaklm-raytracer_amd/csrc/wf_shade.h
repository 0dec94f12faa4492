// wf_shade.h — a path's state between two ray queries (PathRegs, PathRegsL), shade_step, and the kernels that
// are little more than it: wf_shade and the tail finisher wf_finish.
// A part of wavefront.hip's translation unit (included there, once, in the order wf_state.h,
// wf_queue_kernels.h, wf_shade.h, wf_finish_kernels.h, wf_long.h): not for use elsewhere.
#pragma once

namespace {

// a ? x : y of two Vec3D values (a conditional of two lvalues selects their
// ADDRESSES, which keeps the path state in scratch memory)
__device__ __forceinline__ Vec3D pick(bool a, Vec3D x, Vec3D y)
{
    return rt_v3(a ? x.x : y.x, a ? x.y : y.y, a ? x.z : y.z);
}

// the state of one pixel's path between two ray queries
struct PathRegs {
    uint32_t slot;
    bool shadow, inside;
    bool dual;     // the roulette after this path's pending shadow ray was drawn when it was set up
    bool ext_live; // ... and let the path continue: its extension ray (ro, cont) is pending too
    int prev_type, depth, passes_left, light;
    uint32_t rng;
    Vec3D T, L, rp, cont, snorm, ro, rd;
};

// (wf_finish_bvh) a NEE set-up's state — light point, continuation, shading normal, light — in LDS
// between the set-up and its shadow ray's shading: written once and read once per diffuse bounce, it
// holds no registers through the traversal.  Addressed from a wave-uniform base plus the lane id
// recomputed at use (lane_id_here), so no per-lane address stays live either.
struct LdsV3 {
    float *w; // wave-uniform: this wave's column 0 of three WF_BLOCK-strided rows
    __device__ __forceinline__ operator Vec3D() const
    {
        const int l = lane_id_here();
        return rt_v3(w[l], w[WF_BLOCK + l], w[2 * WF_BLOCK + l]);
    }
    __device__ __forceinline__ LdsV3 &operator=(Vec3D v)
    {
        const int l = lane_id_here();
        w[l] = v.x;
        w[WF_BLOCK + l] = v.y;
        w[2 * WF_BLOCK + l] = v.z;
        return *this;
    }
    __device__ __forceinline__ LdsV3 &operator=(const LdsV3 &o) { return *this = (Vec3D)o; }
};
struct LdsInt {
    int *w;
    __device__ __forceinline__ operator int() const { return w[lane_id_here()]; }
    __device__ __forceinline__ LdsInt &operator=(int v)
    {
        w[lane_id_here()] = v;
        return *this;
    }
    __device__ __forceinline__ LdsInt &operator=(const LdsInt &o) { return *this = (int)o; }
};
// PathRegs with the NEE state in LDS (the same fields: shade_step and the load / store helpers take either)
struct PathRegsL {
    uint32_t slot;
    bool shadow, inside, dual, ext_live;
    int prev_type, depth, passes_left;
    LdsInt light;
    uint32_t rng;
    Vec3D T, L;
    LdsV3 rp, cont, snorm;
    Vec3D ro, rd;
};

// (ST: WfState, or the kernel's own copy of it read in place — wf_state.h wf_cold_state)
template <typename ST, typename P>
__device__ __forceinline__ void load_regs(const ST &st, const RtDevFrame &fr, uint32_t slot, P &p)
{
    p.slot = slot;
    const uint32_t flags = st.flags[slot];
    p.shadow = flags & 1u;
    p.inside = (flags >> 1) & 1u;
    p.prev_type = (int)((flags >> 2) & 7u);
    p.dual = (flags >> 5) & 1u;
    p.ext_live = (flags >> 6) & 1u;
    p.depth = (int)(flags >> 8);
    p.rng = fr.rng[slot];
    p.T = st.T[slot];
    p.L = st.L[slot];
    p.passes_left = st.passes_left[slot];
    if (p.shadow) {
        p.light = st.light[slot];
        p.rp = st.rp[slot];
        p.cont = st.cont[slot];
        p.snorm = st.snorm[slot];
    }
}

template <typename ST, typename P>
__device__ __forceinline__ void store_regs(const ST &st, const RtDevFrame &fr, const P &p)
{
    const uint32_t slot = p.slot;
    fr.rng[slot] = p.rng;
    st.T[slot] = p.T;
    st.L[slot] = p.L;
    st.passes_left[slot] = p.passes_left;
    st.flags[slot] = (p.shadow ? 1u : 0u) | (p.inside ? 2u : 0u) | ((uint32_t)p.prev_type << 2) |
                     (p.dual ? 0x20u : 0u) | (p.ext_live ? 0x40u : 0u) | ((uint32_t)p.depth << 8);
    if (p.shadow) {
        st.light[slot] = p.light;
        st.rp[slot] = p.rp;
        st.cont[slot] = p.cont;
        st.snorm[slot] = p.snorm;
    }
}

// a path of a path list with its first pending ray in p.ro / p.rd (the
// shadow ray if one is pending: its direction recomputed as it was set up)
template <typename ST, typename P>
__device__ __forceinline__ void first_ray(const ST &st, const RtDevFrame &fr, uint32_t slot, P &p)
{
    load_regs(st, fr, slot, p);
    p.ro = st.ro[slot];
    p.rd = p.shadow ? rt_normalize(p.rp - p.ro) : st.cont[slot];
}

// One event of trace_path (rt/path_tracing.cuh:268-325) for the hit of the
// ray p.ro/p.rd: emission, BSDF, NEE set-up, roulette, accumulation and the
// pixel's next pass.  Returns true with the next ray in p.ro/p.rd.
//
// DUAL (the queue kernels): when NEE sets up a shadow ray, the Russian
// roulette that the reference draws after the shadow ray (:309-318) is drawn
// right away — nothing between consumes random numbers or changes the
// throughput — so the extension ray (p.ro, p.cont) can be traced in the SAME
// queue iteration as the shadow ray (p.dual, p.ext_live).  The shadow result
// is still applied first (L += direct * T, then T /= p), in the reference's
// order.  Any shade_step (DUAL or not) resumes such a path correctly.
//
// The shadow result and the regeneration are path_event.h's; the bounce is
// path_bounce's text, kept here because calling the helper changes the register
// allocation of wf_shade and of every finisher (profiles/path_event).
template <bool COUNT, bool DUAL = false, typename P>
__device__ __forceinline__ bool shade_step(const RtDevScene &sc, const RtDevFrame &fr, const RtDevCamera &cam,
                                           P &p, int hit, float bx, float by, float bz, int limit, Cnt &c)
{
    bool finish = false, roulette = true, want = false;
    if (!p.shadow) {
        if (hit < 0) {
            finish = true; // miss: break without roulette (:303-306)
            roulette = false;
        } else {
            Surface s;
            shade<COUNT>(sc, hit, bx, by, bz, p.rd, s, c);
            if (p.prev_type != DIFFUSE) p.L = p.L + s.emittance * p.T; // :285-288
            Vec3D nd, w;
            p.prev_type = scatter(p.rd, p.inside, p.rng, s, nd, w);
            p.T = p.T * w;
            p.ro = s.position;
            p.rd = nd;
            if (p.prev_type == DIFFUSE) { // sample_direct_light (:235-265)
                if (COUNT) c.v[RT_CNT_NEE]++;
                float xi = rng_next(p.rng);
                if (sc.light_count == 0) {
                    rng_next(p.rng);
                    rng_next(p.rng);
                    p.L = p.L + rt_v3(0.0f, 0.0f, 0.0f) * p.T;
                } else {
                    p.light = sc.lights[(int)(xi * (float)sc.light_count)];
                    p.rp = light_point(sc, p.light, p.rng);
                    p.cont = p.rd;
                    p.snorm = s.normal;
                    p.rd = rt_normalize(p.rp - p.ro);
                    p.shadow = true;
                    roulette = false; // roulette after the shadow ray
                    want = true;
                    if (DUAL) { // the roulette now (the same draw as after the shadow ray)
                        const float pr = fmaxf(p.T.x, fmaxf(p.T.y, p.T.z));
                        const float r = rng_next(p.rng);
                        p.dual = true;
                        p.ext_live = false;
                        if (!(r > pr)) {
                            if (p.depth == limit) { // max_depth / watchdog before the next extension ray
                                if (COUNT && fr.max_depth <= 0) c.v[RT_CNT_WATCHDOG]++;
                                dev_record_cut(fr);
                            } else {
                                ++p.depth;
                                p.ext_live = true;
                            }
                        }
                    }
                }
            }
        }
    } else {
        path_shadow_result<COUNT>(sc, p, hit, bx, by, bz, c);
        if (p.dual) { // the roulette was drawn at the set-up
            p.dual = false;
            roulette = false;
            if (p.ext_live) {
                p.T = p.T * (1.0f / fmaxf(p.T.x, fmaxf(p.T.y, p.T.z)));
                want = true; // depth was advanced at the set-up
            } else {
                finish = true;
            }
            p.ext_live = false;
        }
    }
    if (roulette) { // Russian roulette (:309-318)
        float pr = fmaxf(p.T.x, fmaxf(p.T.y, p.T.z));
        float r = rng_next(p.rng);
        if (r > pr) {
            finish = true;
        } else {
            p.T = p.T * (1.0f / pr);
            if (p.depth == limit) { // max_depth / watchdog before the next extension ray
                if (COUNT && fr.max_depth <= 0) c.v[RT_CNT_WATCHDOG]++;
                dev_record_cut(fr);
                finish = true;
            } else {
                ++p.depth;
                want = true;
            }
        }
    }
    if (finish) { // accumulation (:322-324), then the pixel's next pass
        if (COUNT) c.path_end(p.depth);
        dev_record_end(fr, p.depth);
        const uint32_t slot = p.slot;
        Vec3D fb = fr.fb[slot] + p.L;
        float sq = fr.sq[slot] + rt_square(rt_luminance(p.L));
        int count = fr.count[slot] + 1;
        fr.fb[slot] = fb;
        fr.sq[slot] = sq;
        fr.count[slot] = count;
        if (p.passes_left > 0) {
            want = start_sample<COUNT>(fr, cam, (int)slot, p.passes_left, p.rng, fb, sq, count, p.ro, p.rd, c);
            if (want) {
                path_begin(p, 1);
            }
        }
    }
    return want;
}

} // namespace

template <bool COUNT>
__global__ void __launch_bounds__(WF_TBLOCK, WF_SHADE_WAVES) wf_shade(RtDevScene sc, RtDevFrame fr, RtDevCamera cam, WfState st, int q)
{
    if (WF_SHADE_PRIO > 0) __builtin_amdgcn_s_setprio(WF_SHADE_PRIO); // ahead of co-resident trace waves
    Cnt c;
    if (COUNT) c.zero();
    const uint32_t n = st.counts[6 + q]; // paths with rays in ray queue q
    const int qn = q ^ 1;
    const int limit = fr.max_depth > 0 ? fr.max_depth : RT_WATCHDOG_BOUNCES;
    for (uint32_t base = blockIdx.x * WF_TBLOCK; base < n; base += gridDim.x * WF_TBLOCK) {
        const uint32_t i = base + threadIdx.x;
        bool want = false;
        PathRegs p;
        p.slot = 0;
        p.shadow = p.ext_live = false;
        p.ro = p.rd = p.cont = rt_v3(0, 0, 0);
        if (i < n) {
            const uint32_t slot = st.q_slot[q][i];
            load_regs(st, fr, slot, p);
            p.ro = st.ro[slot];
            if (p.shadow) {
                // the shadow ray (set up DUAL: its roulette is drawn) and, if the
                // path went on, its extension ray were traced in this iteration
                const bool both = p.ext_live;
                p.rd = rt_normalize(p.rp - p.ro); // the shadow ray's direction, as set up
                const RtF4 h = ldf4(st.hits + st.e_sh[slot]);
                want = shade_step<COUNT, true>(sc, fr, cam, p, __float_as_int(h.x), h.y, h.z, h.w, limit, c);
                if (both) { // p.ro / p.rd = the extension ray: its hit is in too
                    const RtF4 g = ldf4(st.hits + st.e_ext[slot]);
                    want = shade_step<COUNT, true>(sc, fr, cam, p, __float_as_int(g.x), g.y, g.z, g.w, limit, c);
                }
            } else {
                p.rd = st.cont[slot];
                const RtF4 h = ldf4(st.hits + st.e_ext[slot]);
                want = shade_step<COUNT, true>(sc, fr, cam, p, __float_as_int(h.x), h.y, h.z, h.w, limit, c);
            }
            store_regs(st, fr, p);
            if (want) { // the pending ray(s): extension = (ro, cont)
                st.ro[slot] = p.ro;
                st.cont[slot] = pick(p.shadow, p.cont, p.rd);
            }
        }
        const bool to_long = want && st.long_depth > 0 && p.depth > st.long_depth;
        const bool go = want && !to_long;
        const bool sh = go && p.shadow, ex = go && (!p.shadow || p.ext_live);
        const uint32_t es = enqueue_ray(st, qn, sh, p.ro, p.rd);
        const uint32_t ee = enqueue_ray(st, qn, ex, p.ro, pick(p.shadow, p.cont, p.rd));
        if (sh) st.e_sh[p.slot] = es;
        if (ex) st.e_ext[p.slot] = ee;
        enqueue_path(st, qn, go, p.slot);
        // wf_long takes the path with its first pending ray (the shadow ray if any)
        if (__any(to_long)) publish_long(st, to_long, p.slot, p.ro, p.rd);
    }
    if (COUNT) flush_counters(c, fr.counters);
}

// Tail finisher: once few paths remain, each remaining pixel is run to the end
// of its passes by one lane (trace + shade in registers, megakernel style), so
// the long total-internal-reflection paths cost one launch instead of one
// trace/shade iteration per bounce.
template <bool COUNT>
__global__ void __launch_bounds__(WF_BLOCK) wf_finish(RtDevScene sc, RtDevFrame fr, RtDevCamera cam, WfState st, int q)
{
    __shared__ uint32_t s_node[WF_LDS_STACK * WF_BLOCK];
    __shared__ float s_entry[WF_LDS_STACK * WF_BLOCK];
    const int tid = threadIdx.x;
    const int gtid = blockIdx.x * WF_BLOCK + tid;
    Stack<WF_LDS_STACK> stk{s_node + tid, s_entry + tid, WF_BLOCK, st.spill + gtid, st.spill_threads};
    Cnt c;
    if (COUNT) c.zero();
    const uint32_t n = st.counts[6 + q]; // paths of path list q
    const int limit = fr.max_depth > 0 ? fr.max_depth : RT_WATCHDOG_BOUNCES;
    for (uint32_t base = blockIdx.x * WF_BLOCK; base < n; base += gridDim.x * WF_BLOCK) {
        const uint32_t e = base + tid;
        if (e < n) {
            PathRegs p;
            first_ray(st, fr, st.q_slot[q][e], p);
            while (true) {
                float bx = 0.0f, by = 0.0f, bz = 0.0f;
                const int hit = trace<COUNT>(sc, p.ro, p.rd, bx, by, bz, stk, c);
                if (!shade_step<COUNT>(sc, fr, cam, p, hit, bx, by, bz, limit, c)) break;
            }
            store_regs(st, fr, p);
        }
    }
    if (COUNT) {
        flush_counters(c, fr.counters);
        flush_finish_counters(c, fr.counters);
    }
}
